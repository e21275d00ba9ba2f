"""Restatements, from their definitions, of the U-Net glue operations of
csrc/unet_ops.hip (paig_maxpool2_fwd / _fwd_codes / _bwd_relu, paig_upsample2_fwd
/ _bwd), the input generators of their tests and the shapes those tests use.
No aten pooling or interpolation inside: tests/test_unet_glue_ref_cpu.py holds
these against F.max_pool2d, F.interpolate and their autograd first, then
tests/test_gpu_unet_glue.py holds the kernels against these.

Every function takes and returns CPU tensors [F][C][H][W].  The pool keeps the
dtype of its input (its results are selections and, in the backward, one IEEE
add per element: the kernel's bits are determined); the upsample computes in
float64 and also returns sum |w| |v| per element, the scale of its rounding
bound."""
import torch

# ------------------------------------------------------------------- shapes --
# (H, W) of the pool tests and (Hs, Ws) of the upsample tests, F and C of both;
# the CPU test runs the reference against aten on every one of them
POOL_HW = [(2, 4), (4, 8), (6, 12), (2, 2), (6, 6), (18, 18), (5, 7), (5, 8)]
CODE_HW = [(2, 2), (4, 8), (6, 6), (18, 18)]
POOL_FC = [(1, 3), (3, 3), (1, 12), (3, 12)]
UP_HW = [(1, 1), (3, 5), (9, 9), (1, 2), (2, 4), (3, 8), (5, 16), (2, 64), (2, 128), (2, 6), (18, 18), (3, 12),
         (1, 256)]
UP_FC = [(1, 1), (3, 1), (1, 5), (3, 5)]
PARTIAL_WAVE = (3, 8, (1, 3))   # (Hs, Ws, (F, C)): 36 work items of the vector upsample backward

# The second trip of the grid-stride loops: grids stop at 8192 blocks of 256
# threads, so C = 2, the smallest frame of each kernel form and frames enough
# for one full trip plus about 1000 work items (nv or n of the entry point).
TRIP = 8192 * 256
SECOND = [
    # id,                           kernel,      H, W, work items per frame, form
    ("maxpool_fwd_v_k-2x4", "pool_fwd", 2, 4, 2 * 1 * 1, "vector"),
    ("maxpool_fwd_k-2x2", "pool_fwd", 2, 2, 2 * 1 * 1, "scalar"),
    ("maxpool_fwd_codes_k-2x2", "pool_codes", 2, 2, 2 * 1 * 1, None),
    ("maxpool_bwd_relu_v_k-2x4", "pool_bwd", 2, 4, 2 * 1 * 1, "vector"),
    ("maxpool_bwd_relu_k-2x2", "pool_bwd", 2, 2, 2 * 2 * 2, "scalar"),
    ("upsample_fwd_k-1x1", "up_fwd", 1, 1, 2 * 2 * 2, None),
    ("upsample_bwd_k-1x1", "up_bwd", 1, 1, 2 * 1 * 1, "scalar"),
    ("upsample_bwd_v_k-shuffle-1x4", "up_bwd", 1, 4, 2 * 1 * 2, "shuffle"),
]


def frames_for(items_per_frame):
    """the fewest frames past one full trip plus about 1000 work items"""
    F = -(-(TRIP + 1000) // items_per_frame)
    assert TRIP + 1000 <= F * items_per_frame < TRIP + 1000 + items_per_frame
    return F


def rng(H, W, fc):
    """The generator of a case's inputs.  Both test files draw from it in the
    same order (x or s first), so the tensors whose properties the CPU test
    asserts are the ones the kernels are given."""
    return torch.Generator().manual_seed(1000 * H + 10 * W + 7 * fc[0] + fc[1])


# --------------------------------------------------------------------- pool --
def _taps(x):
    """the four pixels of every 2 x 2 window in scan order (y, x), (y, x+1),
    (y+1, x), (y+1, x+1); floor sizes: a trailing odd row / column is ignored"""
    H, W = x.shape[-2] // 2 * 2, x.shape[-1] // 2 * 2
    return [x[..., 0:H:2, 0:W:2], x[..., 0:H:2, 1:W:2], x[..., 1:H:2, 0:W:2], x[..., 1:H:2, 1:W:2]]


def pool_fwd(x):
    """-> (pooled [F][C][H/2][W/2], argmax 0..3): m = first pixel, then each
    later pixel v replaces it where v > m or isnan(v)"""
    t = _taps(x)
    m = t[0].clone()
    am = torch.zeros(m.shape, dtype=torch.int64)
    for k in (1, 2, 3):
        take = (t[k] > m) | torch.isnan(t[k])
        m = torch.where(take, t[k], m)
        am = torch.where(take, torch.full_like(am, k), am)
    return m, am


def pool_codes(x):
    """-> uint8 [F][ceil(C/8)][H/2][W/2][8]: channel c's byte at [c / 8][..][c % 8];
    bits 0..3 = (value > 0) of the window's four pixels, bits 4..5 = the argmax.
    The bytes of the padding channels of the last group are left 0 here and are
    unspecified in the kernel (never written)."""
    F, C = x.shape[:2]
    _, am = pool_fwd(x)
    code = am << 4
    for k, v in enumerate(_taps(x)):
        code = code | ((v > 0).to(torch.int64) << k)
    G = (C + 7) // 8
    out = torch.zeros(F, G * 8, *am.shape[2:], dtype=torch.uint8)
    out[:, :C] = code.to(torch.uint8)
    return out.view(F, G, 8, *am.shape[2:]).permute(0, 1, 3, 4, 2).contiguous()


def codes_by_channel(code, C):
    """[F][G][Ho][Wo][8] -> [F][C][Ho][Wo], the padding channels dropped"""
    F, G, Ho, Wo, _ = code.shape
    return code.permute(0, 1, 4, 2, 3).reshape(F, G * 8, Ho, Wo)[:, :C]


def pool_bwd_relu(x, dy, dx0):
    """(dx0 + dy scattered to each window's argmax) * (x > 0) in the dtype of
    dx0: one add per argmax element, none elsewhere"""
    _, am = pool_fwd(x)
    g = dx0.clone()
    for k, v in enumerate(_taps(g)):
        v.copy_(torch.where(am == k, v + dy, v))
    return torch.where(x > 0, g, torch.zeros_like(g))


# ----------------------------------------------------------------- upsample --
def up_matrix(n):
    """[2n][n] float64: row d holds the two bilinear taps of output d
    (align_corners=False): src = max(0, (d + 0.5) / 2 - 0.5), i0 = floor(src),
    i1 = min(i0 + 1, n - 1), weights 1 - (src - i0) and src - i0"""
    M = torch.zeros(2 * n, n, dtype=torch.float64)
    for d in range(2 * n):
        src = max(0.0, (d + 0.5) * 0.5 - 0.5)
        i0 = int(src)
        i1 = min(i0 + 1, n - 1)
        M[d, i0] += 1.0 - (src - i0)
        M[d, i1] += src - i0
    return M


def up_fwd(s):
    """-> (u [F][C][2Hs][2Ws], sum |w| |s|) in float64"""
    My, Mx = up_matrix(s.shape[-2]), up_matrix(s.shape[-1])
    f = lambda v: torch.einsum("yi,fcij,xj->fcyx", My, v, Mx)   # noqa: E731
    return f(s.double()), f(s.double().abs())


def up_bwd(du, s=None):
    """-> (ds [F][C][Hs][Ws], sum |w| |du|) in float64; s given: both times (s > 0)"""
    My, Mx = up_matrix(du.shape[-2] // 2), up_matrix(du.shape[-1] // 2)
    f = lambda v: torch.einsum("yi,fcyx,xj->fcij", My, v, Mx)   # noqa: E731
    ds, a = f(du.double()), f(du.double().abs())
    if s is not None:
        keep = (s > 0).double()
        ds, a = ds * keep, a * keep
    return ds, a


# --------------------------------------------------------------- generators --
def _plant_zeros(x):
    """an exact 0.0 and a -0.0 (flat elements 0 and 1) where there is room"""
    v = x.view(-1)
    if v.numel() >= 2:
        v[0], v[1] = 0.0, -0.0
    return x


def ties(g, *shape):
    """integers in {-1, 0, 1, 2} as fp32: most windows have a tied maximum, half
    the values are <= 0 (the ReLU' mask)"""
    return _plant_zeros(torch.randint(-1, 3, shape, generator=g).float())


def gauss(g, *shape):
    """standard normal fp32 with an exact 0.0 and a -0.0: about half <= 0"""
    return _plant_zeros(torch.randn(*shape, generator=g))


def with_nans(g, F, C, H, W):
    """gauss with a NaN at each of the four window positions (position k in
    window k mod the window count: with fewer than 4 windows some hold two)"""
    x = gauss(g, F, C, H, W)
    t = _taps(x)
    n = t[0].numel()
    for k in range(4):
        w = k % n
        idx = []
        for d in reversed(t[k].shape):
            idx.append(w % d)
            w //= d
        t[k][tuple(reversed(idx))] = float("nan")
    return x
