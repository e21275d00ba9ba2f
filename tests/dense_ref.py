"""Plain float64 restatements of the small fused operations between the U-Net
and the decoder, forward and hand-written backward, written from
include/paig_hip.h and the reference lines it cites (nn/network/blocks.py):
the velocity encoder (:22-48), VariableFromNetwork (:311-322), the localiser's
dense tail and position head (:98-102), the mask softmax (:84-96), the
velocity packing and the column sum.  The GPU tests of the kernels compare
with these; tests/test_dense_ref_cpu.py checks every backward here against
torch autograd first.

Every function takes and returns CPU tensors and computes in the dtype of its
inputs (float64 in the tests).  The forwards are built from differentiable
torch operations; the backwards use no autograd."""
import torch

HID = 100   # velocity MLP hidden width (blocks.py:24-28)
VH = 200    # VariableFromNetwork hidden width (blocks.py:314)
VIN = 10    # its input, ones[1, 10] (blocks.py:319)


# ---------------------------------------------------------- velocity packing --
def vel_pack(pos, K, S, alt=0):
    """pos [B][Te][2K] -> X[k*B + b][2t + j] = pos[b][t][2k + j], t < S
    (blocks.py:43-45); alt (blocks.py:33-38): pos[b][t+1] - pos[b][t], t < S-1."""
    B = pos.shape[0]
    d = pos[:, 1:S] - pos[:, :S - 1] if alt else pos[:, :S]
    n = d.shape[1]
    return d.reshape(B, n, K, 2).permute(2, 0, 1, 3).reshape(K * B, 2 * n)


def vel_unpack(dX, dpos0, B, Te, K, S, alt=0):
    """The adjoint of vel_pack (+ dpos0 [B][2K] at step S-1): the gradient that
    paig_vel_unpack_add adds to dpos [B][Te][2K].  dX, dpos0: None = absent."""
    ref = dX if dX is not None else dpos0
    g = torch.zeros(B, Te, 2 * K, dtype=ref.dtype)
    if dX is not None:
        n = S - 1 if alt else S
        d = dX.reshape(K, B, n, 2).permute(1, 2, 0, 3).reshape(B, n, 2 * K)
        if alt:
            g[:, 1:S] += d
            g[:, :S - 1] -= d
        else:
            g[:, :S] += d
    if dpos0 is not None:
        g[:, S - 1] += dpos0
    return g


# -------------------------------------------------------------- velocity MLP --
def velmlp_fwd(pos, K, S, W0, b0, W2, b2, W4, b4):
    """-> X [K*B][2S], h1, h2 [K*B][100], vel [K*B][2]"""
    X = vel_pack(pos, K, S)
    h1 = torch.tanh(X @ W0.T + b0)
    h2 = torch.tanh(h1 @ W2.T + b2)
    return X, h1, h2, h2 @ W4.T + b4


def velmlp_bwd(dvel, X, h1, h2, W0, W2, W4):
    """-> dX, [dW0, db0, dW2, db2, dW4, db4] (the slab row's order)"""
    dz2 = (dvel @ W4) * (1 - h2 * h2)
    dz1 = (dz2 @ W2) * (1 - h1 * h1)
    return dz1 @ W0, [dz1.T @ X, dz1.sum(0), dz2.T @ h1, dz2.sum(0), dvel.T @ h2, dvel.sum(0)]


# ------------------------------------------------------ VariableFromNetwork --
def vfn_fwd(W1, b1, W2, b2):
    """-> h [200], y [P], sigmoid(y)"""
    h = torch.tanh(W1 @ torch.ones(VIN, dtype=W1.dtype) + b1)
    y = W2 @ h + b2
    return h, y, torch.sigmoid(y)


def vfn_bwd(d, y, sig, h, W2):
    """d: the adjoint of y (sig = 0) or of sigmoid(y) (sig = 1).
    -> dW1 [200][10], db1, dW2 [P][200], db2, dh [200] (before the tanh')"""
    if sig:
        s = torch.sigmoid(y)
        d = d * s * (1 - s)
    dh = W2.T @ d
    g = dh * (1 - h * h)
    return g[:, None].expand(VH, VIN).clone(), g, torch.outer(d, h), d, dh


# ------------------------------------------------------ position head, tail --
def pos_head_fwd(h3, N, K, half):
    """pos[f][2k + j] = tanh(h3[k*N + f][j]) * half + half (blocks.py:101-102)"""
    return (torch.tanh(h3) * half + half).reshape(K, N, 2).permute(1, 0, 2).reshape(N, 2 * K)


def pos_head_bwd(h3, dpos, N, K, half):
    t = torch.tanh(h3)
    return dpos.reshape(N, K, 2).permute(1, 0, 2).reshape(K * N, 2) * half * (1 - t * t)


def head_fwd(h2, W3, b3, F, K, half):
    """-> h3 [K*F][2], pos [F][2K] (blocks.py:100-102)"""
    h3 = h2 @ W3.T + b3
    return h3, pos_head_fwd(h3, F, K, half)


def head_bwd(h2, h3, dpos, W3, F, K, half, vel=None):
    """-> dh2 (l2's ReLU' applied), dW3 [2][IN], db3 [2].  vel = (dX, dpos0, B,
    Te, S, alt): the velocity encoder's input gradient added to dpos first."""
    if vel is not None:
        dX, dpos0, B, Te, S, alt = vel
        dpos = dpos + vel_unpack(dX, dpos0, B, Te, K, S, alt).reshape(F, 2 * K)
    dh3 = pos_head_bwd(h3, dpos, F, K, half)
    return (dh3 @ W3) * (h2 > 0), dh3.T @ h2, dh3.sum(0)


def l2_bwd(dh2, W2, h1):
    """l2's data gradient with l1's ReLU' (blocks.py:98-99)"""
    return (dh2 @ W2) * (h1 > 0)


def dense_tail_fwd(part, b1, W2, b2, W3, b3, F, K, half):
    """part [S][K*F][IN] -> h1, h2, h3, pos (blocks.py:98-102)"""
    h1 = torch.relu(part.sum(0) + b1)
    h2 = torch.relu(h1 @ W2.T + b2)
    return (h1, h2) + head_fwd(h2, W3, b3, F, K, half)


# -------------------------------------------------------------- mask softmax --
def mask_softmax_fwd(logits, x, pool=False):
    """logits [F][K][H][W], x [F][C][H][W] -> masks [F][K+1][H][W], objs
    [K*F][C][H][W] (object k's frames first), AvgPool2d(2) of objs or None
    (blocks.py:84-96)."""
    F, K, H, W = logits.shape
    masks = torch.softmax(torch.cat([logits, torch.ones(F, 1, H, W, dtype=logits.dtype)], 1), 1)
    objs = torch.cat([masks[:, k:k + 1] * x for k in range(K)], 0)
    pobjs = None
    if pool:
        pobjs = (objs[:, :, 0::2, 0::2] + objs[:, :, 0::2, 1::2] + objs[:, :, 1::2, 0::2] + objs[:, :, 1::2, 1::2]) / 4
    return masks, objs, pobjs


def mask_softmax_bwd(logits, x, masks, dobjs, flags=0):
    """flags 1: the logits are a ReLU's output (its derivative applied), 2:
    dobjs is the gradient of the pooled objects.  -> dlogits"""
    F, K, H, W = logits.shape
    if flags & 2:
        dobjs = dobjs.repeat_interleave(2, 2).repeat_interleave(2, 3) / 4
    dm = (dobjs.reshape(K, F, -1, H, W) * x[None]).sum(2).permute(1, 0, 2, 3)   # [F][K][H][W]
    m = masks[:, :K]
    dl = m * (dm - (m * dm).sum(1, keepdim=True))
    return dl * (logits > 0) if flags & 1 else dl


# ---------------------------------------------------------------- column sum --
def colsum(X, out0=None):
    """out[n] = sum_r X[r][n] (+ out0)"""
    s = X.sum(0)
    return s if out0 is None else s + out0
