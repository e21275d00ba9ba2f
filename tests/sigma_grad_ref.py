"""tests/sigma_ref.py's decoder restated with the attention-window scale as a
TENSOR that can carry a gradient (the reference's sigma is a Python float and
has none: its original trainable ``logsigma`` survives only as a comment,
physics_models.py:155-161).  The yardstick of dL/dsigma is autograd through
this restatement.

What changes against sigma_ref (which stays as it is):
  * sigma is a float64 tensor: 0-dim / [1] (one scale), or [N] (one per frame,
    so that ONE backward yields every frame's dL/dsigma_f);
  * theta0 = theta4 = sigma.expand(N) (float64, as torch.tensor([sigma]) tiled);
  * theta2 / theta5 are multiplied by sigma in the positions' dtype: for the
    model's fp32 positions that is ``sigma.to(torch.float32)``, the scalar
    multiply sigma_ref's ``tensor * numpy_float64`` performs; float64
    positions (the float64 yardstick) keep sigma exact, as sigma_ref does.
Everything else is sigma_ref's, line for line.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from oracle import physics_oracle as O

LN2 = math.log(2.0)


def sigma_from_u(u):
    """sigma = exp(ln 2 tanh(u)) in float64 from the parameter u (any float dtype)."""
    return torch.exp(LN2 * torch.tanh(u.to(torch.float64)))


def _warp(joint_k, loc, h, H, sigma):
    N = loc.shape[0]
    s = sigma.to(torch.float64).expand(N)
    zero = torch.tile(torch.tensor([0.0]), [N])
    sl = sigma.to(loc.dtype)
    t2 = (H / 2 - loc[:, 0]) / h * sl
    t5 = (H / 2 - loc[:, 1]) / h * sl
    theta = torch.stack([s, zero, t2, zero, s, t5], 1).view(-1, 2, 3)
    grid = F.affine_grid(theta, [N, 6, H, H], align_corners=False)
    src = joint_k.expand(N, -1, -1, -1)
    return F.grid_sample(src, grid.to(src.dtype), mode="bilinear", padding_mode="zeros", align_corners=False), grid


def _objects(cfg, joint, pos, sigma):
    K, h, H = cfg.n_objs, cfg.tmpl, cfg.size
    outs = []
    for k in range(K):
        o, _ = _warp(joint[k:k + 1], pos[:, 2 * k:2 * k + 2], h, H, sigma)
        outs.append((o[:, :3], o[:, 3:]))
    return outs


def st_decoder_sigma(cfg, joint, bg, pos, sigma):
    """sigma_ref.st_decoder_sigma with sigma a float64 tensor (0-dim, [1] or [N])."""
    K, N = cfg.n_objs, pos.shape[0]
    outs = _objects(cfg, joint, pos, sigma)
    masks = torch.stack([t - 5 for t, _ in outs] + [torch.ones_like(outs[0][0])], 1)
    masks = torch.softmax(masks, 1)
    conts = [c for _, c in outs] + [bg.expand(N, -1, -1, -1)]
    return sum(masks[:, i] * conts[i] for i in range(K + 1))


def st_decoder_parts_sigma(cfg, joint, bg, pos, sigma):
    N = pos.shape[0]
    outs = _objects(cfg, joint, pos, sigma)
    contents = [c for _, c in outs] + [bg.expand(N, -1, -1, -1)]
    masks = torch.softmax(torch.stack([t - 5 for t, _ in outs] + [torch.ones_like(outs[0][0])], 1), 1)
    return contents, torch.unbind(masks, 1)


@contextlib.contextmanager
def patched_oracle(sigma):
    """sigma_ref.patched_oracle with a tensor sigma (e.g. sigma_from_u(u) of a
    leaf u that requires grad: O.train_step's backward then leaves d loss / du
    in u.grad)."""
    old = O.st_decoder, O.st_decoder_parts
    O.st_decoder = lambda cfg, joint, bg, pos: st_decoder_sigma(cfg, joint, bg, pos, sigma)
    O.st_decoder_parts = lambda cfg, joint, bg, pos: st_decoder_parts_sigma(cfg, joint, bg, pos, sigma)
    try:
        yield sigma
    finally:
        O.st_decoder, O.st_decoder_parts = old
