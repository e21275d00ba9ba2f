"""The black-box rollout cell (lstm_ode_cell) restated in plain torch, in the
dtype of its inputs: the reference the HIP kernels paig_rollout_lstm_fwd /
_bwd and the whole step are checked against (test infrastructure).

    x = [(pos - s) / s, vel / s]                       s = frame side / 2
    z = W_ih x + b_ih + W_hh h + b_hh                  gates i, f, g, o
    c' = sig(z_f) c + sig(z_i) tanh(z_g);  h' = sig(z_o) tanh(c')
    y = W_p h' + b_p;  pos' = pos + s y[:D];  vel' = vel + s y[D:]

h and c are carried across calls (one call per rollout step); reset() puts
them back to zero, the start of every rollout.
"""
import torch

PFX = "rollout_cell."
KEYS = ("lstm.weight_ih", "lstm.weight_hh", "lstm.bias_ih", "lstm.bias_hh", "proj.weight", "proj.bias")


def key_shapes(D, H):
    return {"lstm.weight_ih": (4 * H, 2 * D), "lstm.weight_hh": (4 * H, H), "lstm.bias_ih": (4 * H,),
            "lstm.bias_hh": (4 * H,), "proj.weight": (2 * D, H), "proj.bias": (2 * D,)}


def default_weights(D, H, seed):
    """A seeded default initialisation in the cell's own rule: torch's draws
    for nn.LSTMCell(2D, H) and nn.Linear(H, 2D), the read-out scaled by 0.1.
    {short key: fp32 tensor}."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lstm = torch.nn.LSTMCell(2 * D, H)
        proj = torch.nn.Linear(H, 2 * D)
    W = {"lstm.weight_ih": lstm.weight_ih, "lstm.weight_hh": lstm.weight_hh, "lstm.bias_ih": lstm.bias_ih,
         "lstm.bias_hh": lstm.bias_hh, "proj.weight": proj.weight * 0.1, "proj.bias": proj.bias * 0.1}
    return {k: v.detach().clone() for k, v in W.items()}


class LstmCellRef:
    """Callable as the oracle's cells are: cell(P, pos, vel) -> (pos, vel), P
    holding the six tensors under ``prefix``."""

    def __init__(self, half, prefix=PFX):
        self.half = half
        self.prefix = prefix
        self.reset()

    def reset(self):
        self.h = self.c = None

    def __call__(self, P, pos, vel):
        W = [P[self.prefix + k] for k in KEYS]
        w_ih, w_hh, b_ih, b_hh, w_p, b_p = W
        H, D = w_hh.shape[1], pos.shape[1]
        s = torch.as_tensor(self.half, dtype=pos.dtype)
        if self.h is None:
            self.h = torch.zeros(pos.shape[0], H, dtype=pos.dtype)
            self.c = torch.zeros(pos.shape[0], H, dtype=pos.dtype)
        x = torch.cat([(pos - s) / s, vel / s], 1)
        z = x @ w_ih.t() + b_ih + self.h @ w_hh.t() + b_hh
        i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), \
            torch.sigmoid(z[:, 3 * H:])
        self.c = f * self.c + i * g
        self.h = o * torch.tanh(self.c)
        y = self.h @ w_p.t() + b_p
        return pos + s * y[:, :D], vel + s * y[:, D:]


def rollout(W, pos0, vel0, R, half):
    """pos_vel_seq [B, R+1, 2D] of R steps from (pos0, vel0) and a zero hidden
    state; W: {short key: tensor} in pos0's dtype."""
    cell = LstmCellRef(half, prefix="")
    pos, vel = pos0, vel0
    seq = [torch.cat([pos, vel], 1)]
    for _ in range(R):
        pos, vel = cell(W, pos, vel)
        seq.append(torch.cat([pos, vel], 1))
    return torch.stack(seq, 1)
