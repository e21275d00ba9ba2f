"""The interaction-network rollout cell (interaction_ode_cell) restated in
plain torch, in the dtype of its inputs: the reference the HIP kernels
paig_rollout_in_fwd / _bwd and the whole step are checked against (test
infrastructure, not a test).

    s_i  = [(pos_i - s) / s, vel_i / s]                  s = frame side / 2, pos_i = pos[:, 2i:2i+2]
    e_ij = tanh(W_r2 tanh(W_r1 [s_i, s_j] + b_r1) + b_r2)    every ordered pair j != i (receiver first)
    a_i  = sum_{j != i} e_ij                             in increasing j
    y_i  = W_o2 tanh(W_o1 [s_i, a_i] + b_o1) + b_o2
    pos_i' = pos_i + s y_i[:2];  vel_i' = vel_i + s y_i[2:]

The cell is memoryless: no hidden state, no dt.
"""
import torch

PFX = "rollout_cell."
KEYS = ("rel.0.weight", "rel.0.bias", "rel.2.weight", "rel.2.bias", "obj.0.weight", "obj.0.bias", "obj.2.weight",
        "obj.2.bias")


def key_shapes(D, H):
    return {"rel.0.weight": (H, 8), "rel.0.bias": (H,), "rel.2.weight": (H, H), "rel.2.bias": (H,),
            "obj.0.weight": (H, 4 + H), "obj.0.bias": (H,), "obj.2.weight": (4, H), "obj.2.bias": (4,)}


def default_weights(D, H, seed):
    """A seeded default initialisation in the cell's own rule: torch's draws
    for the four nn.Linear layers in the cell's construction order, the last
    one scaled by 0.1.  {short key: fp32 tensor}."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lin = {"rel.0": torch.nn.Linear(8, H), "rel.2": torch.nn.Linear(H, H), "obj.0": torch.nn.Linear(4 + H, H),
               "obj.2": torch.nn.Linear(H, 4)}
    W = {}
    for name, m in lin.items():
        scale = 0.1 if name == "obj.2" else 1.0
        W[name + ".weight"] = (m.weight * scale).detach().clone()
        W[name + ".bias"] = (m.bias * scale).detach().clone()
    return {k: W[k] for k in KEYS}


class InCellRef:
    """Callable as the oracle's cells are: cell(P, pos, vel) -> (pos, vel), P
    holding the eight tensors under ``prefix``."""

    def __init__(self, half, prefix=PFX):
        self.half = half
        self.prefix = prefix

    def reset(self):
        pass

    def __call__(self, P, pos, vel):
        w_r1, b_r1, w_r2, b_r2, w_o1, b_o1, w_o2, b_o2 = [P[self.prefix + k] for k in KEYS]
        K = pos.shape[1] // 2
        s = torch.as_tensor(self.half, dtype=pos.dtype)
        st = [torch.cat([(pos[:, 2 * i:2 * i + 2] - s) / s, vel[:, 2 * i:2 * i + 2] / s], 1) for i in range(K)]
        npos, nvel = [], []
        for i in range(K):
            a = None
            for j in range(K):
                if j == i:
                    continue
                h = torch.tanh(torch.cat([st[i], st[j]], 1) @ w_r1.t() + b_r1)
                e = torch.tanh(h @ w_r2.t() + b_r2)
                a = e if a is None else a + e
            y = torch.tanh(torch.cat([st[i], a], 1) @ w_o1.t() + b_o1) @ w_o2.t() + b_o2
            npos.append(pos[:, 2 * i:2 * i + 2] + s * y[:, :2])
            nvel.append(vel[:, 2 * i:2 * i + 2] + s * y[:, 2:])
        return torch.cat(npos, 1), torch.cat(nvel, 1)


def rollout(W, pos0, vel0, R, half):
    """pos_vel_seq [B, R+1, 2D] of R steps from (pos0, vel0); W: {short key:
    tensor} in pos0's dtype."""
    cell = InCellRef(half, prefix="")
    pos, vel = pos0, vel0
    seq = [torch.cat([pos, vel], 1)]
    for _ in range(R):
        pos, vel = cell(W, pos, vel)
        seq.append(torch.cat([pos, vel], 1))
    return torch.stack(seq, 1)
