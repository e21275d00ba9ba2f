"""The oracle's decoder restated with the attention-window scale sigma
(reference nn/network/physics_models.py:160-182, stn.py:5-16), for the tests of
``PhysicsNet.log_sig != 1``.  oracle/physics_oracle.py itself states sigma = 1
and is not edited: ``patched_oracle(sigma)`` swaps these functions into it for
the duration of a test (its forward looks ``st_decoder`` up as a module global).

theta as the reference builds it:
  * sigma = np.exp(np.log(log_sig)), a numpy float64 (exact for 0.5, 1.5, 2;
    other values such as 0.7 may come back an ulp off);
  * theta0 = theta4 = torch.tensor([sigma]) tiled: float64;
  * theta2 = (H/2 - x)/tmpl * sigma, theta5 likewise: the positions' dtype
    (fp32 in the model: a tensor times a numpy scalar is a scalar multiply);
  * torch.stack promotes theta to float64, affine_grid runs in float64 (Q9),
    and the grid is cast to the sources' dtype before grid_sample.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import physics_oracle as O


def sigma_of(log_sig):
    return np.exp(np.log(log_sig))


def _warp(joint_k, loc, h, H, sigma):
    N = loc.shape[0]
    s = torch.tile(torch.tensor([sigma]), [N])
    zero = torch.tile(torch.tensor([0.0]), [N])
    t2 = (H / 2 - loc[:, 0]) / h * sigma
    t5 = (H / 2 - loc[:, 1]) / h * sigma
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
    """O.st_decoder with the window scale sigma (a numpy float64)."""
    K, N = cfg.n_objs, pos.shape[0]
    outs = _objects(cfg, joint, pos, sigma)
    masks = torch.stack([t - 5 for t, _ in outs] + [torch.ones_like(outs[0][0])], 1)
    masks = torch.softmax(masks, 1)
    conts = [c for _, c in outs] + [bg.expand(N, -1, -1, -1)]
    return sum(masks[:, i] * conts[i] for i in range(K + 1))


def st_decoder_parts_sigma(cfg, joint, bg, pos, sigma):
    """O.st_decoder_parts with the window scale sigma."""
    N = pos.shape[0]
    outs = _objects(cfg, joint, pos, sigma)
    contents = [c for _, c in outs] + [bg.expand(N, -1, -1, -1)]
    masks = torch.softmax(torch.stack([t - 5 for t, _ in outs] + [torch.ones_like(outs[0][0])], 1), 1)
    return contents, torch.unbind(masks, 1)


def sample_coords(K, H, pos, sigma):
    """The unnormalised grid_sample coordinates (fp32, as grid_sample forms
    them) of every output pixel: [K][N][H][W][2]."""
    h = H // 2
    out = []
    for k in range(K):
        _, grid = _warp(torch.zeros(1, 6, h, h), pos[:, 2 * k:2 * k + 2], h, H, sigma)
        g = grid.float()
        out.append(((g + 1) * h - 1) / 2)
    return torch.stack(out)


@contextlib.contextmanager
def patched_oracle(log_sig):
    """oracle.physics_oracle with its two decoder functions at sigma =
    exp(log(log_sig)); restored on exit."""
    sigma = sigma_of(log_sig)
    old = O.st_decoder, O.st_decoder_parts
    O.st_decoder = lambda cfg, joint, bg, pos: st_decoder_sigma(cfg, joint, bg, pos, sigma)
    O.st_decoder_parts = lambda cfg, joint, bg, pos: st_decoder_parts_sigma(cfg, joint, bg, pos, sigma)
    try:
        yield sigma
    finally:
        O.st_decoder, O.st_decoder_parts = old
