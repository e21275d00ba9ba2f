"""Addressing of the fused layer backward's prefetch (csrc/conv_bwd.hip,
paig_conv2d_bwd): the staging loads go through buffer descriptors of one
tile's frames, with out-of-range offsets for halo rows, and the per-unit
addressing is formed once per block.  Every operand here is a view inside a
larger allocation, with a frame stride larger than its C x H x W, and
everything around the frames (both ends of the allocation, the gaps between
frames) is NaN (0xFF for the pool's window codes): a halo row or a frame tail
read from a neighbour makes the outputs non-finite.  Results are compared with
the float64 references of tests/test_gpu_conv_bwd.py, at its bars."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err
from test_gpu_conv_bwd import DEV, TOL, XMAX_SLOTS, L, _ref, _xmax_of, p, st

pytestmark = pytest.mark.gpu

NAN = float("nan")
GAP, END = 68, 132   # floats between frames / at both ends (multiples of 4: 16-byte aligned frames)


def _poisoned(t):
    """t [F, ...] as a view with frame stride numel + GAP inside a NaN-filled
    allocation; returns (allocation, view, frame stride)."""
    F_, n = t.shape[0], t[0].numel()
    fs = n + GAP
    buf = torch.full((END + F_ * fs + END,), NAN, device=DEV)
    v = buf[END:END + F_ * fs].view(F_, fs)[:, :n].view(t.shape)
    v.copy_(t)
    return buf, v, fs


def _gaps_untouched(buf, v, fs):
    """Nothing outside the view's frames was written (all still NaN)."""
    F_, n = v.shape[0], v[0].numel()
    body = buf[END:END + F_ * fs].view(F_, fs)
    return bool(torch.isnan(buf[:END]).all() and torch.isnan(buf[END + F_ * fs:]).all()
                and torch.isnan(body[:, n:]).all())


def _launch(x, dy, w, mode, nmax, kind="", relu=True, acc=False, xmax=None, pool=None, code=None, cfs=0):
    """One paig_conv2d_bwd launch on poisoned views of x (UPS: the half-
    resolution source), dy, aux (= x), the pooled gradient and the codes.
    Returns (dx, dw, db) of the view, after checking that nothing was written
    around dx's frames."""
    F_, cin, hx = x.shape[0], x.shape[1], x.shape[2]
    cout, hw = w.shape[0], dy.shape[2]
    bx, vx, xfs = _poisoned(x)
    bd, vd, dfs = _poisoned(dy)
    ba, va, afs = _poisoned(x)      # the ReLU' mask: a view of its own
    bo, vo, ofs = _poisoned(torch.full_like(x, 0.5) if acc else torch.full_like(x, NAN))
    if not acc:
        vo.fill_(NAN)               # write mode: every element of the view must be written
    pp = pc = None
    pfs = cs = 0
    if kind == "pool":
        bp, vp, pfs = _poisoned(pool)
        cs = cfs + 72               # bytes; codes are read as 8-byte words
        bc = torch.full((136 + F_ * cs + 136,), 255, dtype=torch.uint8, device=DEV)
        bc[136:136 + F_ * cs].view(F_, cs)[:, :cfs].copy_(code.view(F_, cfs))
        pp, pc = vp.data_ptr(), bc.data_ptr() + 136
    flags = mode | (2 if relu else 0) | (4 if acc else 0) | {"": 0, "up": 32, "pool": 64}[kind]
    slab = torch.empty(nmax * (cout * cin * 9 + cout), device=DEV)
    nb = ctypes.c_int(0)
    L().paig_conv2d_bwd(vx.data_ptr(), xfs, 0, 0, vd.data_ptr(), dfs, vo.data_ptr(), ofs,
                        va.data_ptr() if relu else None, afs, p(w), p(slab), nmax, ctypes.byref(nb), F_, cin, cout, hw,
                        hw, 3, flags, p(xmax), XMAX_SLOTS if xmax is not None else 0, pp, pfs, pc, cs, None, st())
    g = torch.empty(cout * cin * 9 + cout, device=DEV)
    L().paig_slab_reduce(p(slab), nb.value, g.numel(), g.numel(), p(g), 0, st())
    torch.cuda.synchronize()
    assert _gaps_untouched(bo, vo, ofs), "wrote outside dx's frames"
    n = cout * cin * 9
    return vo.contiguous(), g[:n].view_as(w).clone(), g[n:].clone()


def _operands(cin, cout, hw, F_, hx=None):
    hx = hx or hw
    torch.manual_seed(cin * 1000 + cout * 10 + hw + F_)
    x = torch.relu(torch.randn(F_, cin, hx, hx, device=DEV))
    w = torch.randn(cout, cin, 3, 3, device=DEV) * 0.2
    b = torch.randn(cout, device=DEV) * 0.1
    dy = torch.randn(F_, cout, hw, hw, device=DEV)
    return x, w, b, dy


def _check(got, ref, tol, what):
    dx, gw, gb = got
    rdx, rgw, rgb = ref
    assert torch.isfinite(dx).all() and torch.isfinite(gw).all() and torch.isfinite(gb).all(), what
    ex, ew, eb = rel_err(dx, rdx), rel_err(gw, rgw), rel_err(gb, rgb)
    print(what, f"dx {ex:.2e} dw {ew:.2e} db {eb:.2e}")
    assert ex <= tol, ("dx", what)
    assert ew <= tol, ("dw", what)
    assert eb <= 1e-5, ("db", what)


# frames per tile: 4 at 8 x 8, 1 at 16 x 16 (whole-frame tiles); 32 x 32: four row tiles per frame
@pytest.mark.parametrize("mode", [128, 256])
@pytest.mark.parametrize("cin,cout,hw", [(32, 32, 8), (16, 32, 8), (16, 16, 16), (8, 16, 16), (8, 8, 32), (24, 8, 32)])
def test_plain_frame_tails_and_persistent_walk(cin, cout, hw, mode):
    """F = 1, F not a multiple of the frames per tile, and two persistent
    blocks walking every tile."""
    for F_, nmax in ((1, 512), (6, 512), (7, 2)):
        x, w, b, dy = _operands(cin, cout, hw, F_)
        xmax = _xmax_of(x, w, b, mode) if mode == 128 else None
        got = _launch(x, dy, w, mode, nmax, xmax=xmax)
        _check(got, _ref(x, w, dy, torch.zeros_like(x), x), TOL[mode], (F_, nmax))


@pytest.mark.parametrize("mode", [128, 256])
@pytest.mark.parametrize("cin,cout,hw", [(16, 16, 32), (32, 16, 16), (16, 16, 36), (32, 16, 18)])
def test_upsample_fold(cin, cout, hw, mode):
    """The half-resolution window and its ReLU' mask through descriptors
    (3bp's 36 / 18: rows that are not whole M-tiles)."""
    hs = hw // 2
    for F_, nmax in ((1, 512), (3, 2)):
        xs, w, b, dy = _operands(cin, cout, hw, F_, hs)
        xr = xs.double().cpu().requires_grad_(True)
        wr = w.double().cpu().requires_grad_(True)
        xu = F.interpolate(xr, size=(hw, hw), mode="bilinear", align_corners=False, antialias=True)
        F.conv2d(xu, wr, padding="same").backward(dy.double().cpu())
        ref = (xr.grad * (xs.cpu() > 0), wr.grad, dy.double().cpu().sum((0, 2, 3)))
        xmax = None
        if mode == 128:
            xmax = torch.zeros(XMAX_SLOTS, device=DEV)
            out = torch.empty(F_, cout, hw, hw, device=DEV)
            L().paig_conv2d_fwd_ex(p(xs), cin * hs * hs, 0, 0, p(out), cout * hw * hw, None, 0, p(w), p(b), F_, cin,
                                   cout, hw, hw, 3, 32 | mode, p(xmax), XMAX_SLOTS, st())
        got = _launch(xs, dy, w, mode, nmax, kind="up", xmax=xmax)
        _check(got, ref, TOL[mode], (F_, nmax))


@pytest.mark.parametrize("mode", [128, 256])
@pytest.mark.parametrize("cin,cout,hw", [(8, 8, 32), (16, 16, 16)])
def test_pool_fold(cin, cout, hw, mode):
    """The pooled gradient and the window codes through descriptors."""
    hp = hw // 2
    for F_, nmax in ((1, 512), (5, 2)):
        x, w, b, gy = _operands(cin, cout, hw, F_)
        torch.manual_seed(F_ + mode)
        gp = torch.randn(F_, cout, hp, hp, device=DEV)
        y = torch.empty(F_, cout, hw, hw, device=DEV)
        pool = torch.empty(F_, cout, hp, hp, device=DEV)
        cfs = -(-cout // 8) * 8 * hp * hp
        code = torch.empty(F_ * cfs, dtype=torch.uint8, device=DEV)
        xmax = torch.zeros(XMAX_SLOTS, device=DEV)
        L().paig_conv2d_fwd_pwc(p(x), cin * hw * hw, 0, 0, p(y), cout * hw * hw, None, 0, p(w), p(b), F_, cin, cout,
                                hw, hw, 3, 1 | 64 | mode, p(xmax) if mode == 128 else None,
                                XMAX_SLOTS if mode == 128 else 0, p(pool), cout * hp * hp, p(code), cfs, None, st())
        torch.cuda.synchronize()
        # float64 reference with the GPU forward's own ReLU' masks and argmaxes
        xd, wd, yc = x.double().cpu(), w.double().cpu(), y.cpu()
        _, idx = F.max_pool2d(yc, 2, return_indices=True)
        scat = torch.zeros(F_, cout, hw * hw, dtype=torch.float64)
        scat.scatter_(2, idx.view(F_, cout, -1), gp.double().cpu().view(F_, cout, -1))
        dpre = (yc > 0) * (gy.double().cpu() + scat.view(F_, cout, hw, hw))
        ref = (torch.nn.grad.conv2d_input(xd.shape, wd, dpre, padding=1) * (x.cpu() > 0),
               torch.nn.grad.conv2d_weight(xd, wd.shape, dpre, padding=1), dpre.sum((0, 2, 3)))
        got = _launch(x, gy, w, mode, nmax, kind="pool", xmax=xmax if mode == 128 else None, pool=gp, code=code,
                      cfs=cfs)
        _check(got, ref, TOL[mode], (F_, nmax))


@pytest.mark.parametrize("relu,acc", [(False, True), (True, False), (True, True)])
def test_accumulate_and_mask_flags(relu, acc):
    cin, cout, hw, F_ = 16, 16, 16, 3
    x, w, b, dy = _operands(cin, cout, hw, F_)
    xmax = _xmax_of(x, w, b, 128)
    got = _launch(x, dy, w, 128, 512, relu=relu, acc=acc, xmax=xmax)
    dx0 = torch.full_like(x, 0.5) if acc else torch.zeros_like(x)
    _check(got, _ref(x, w, dy, dx0, x if relu else None), TOL[128], (relu, acc))


@pytest.mark.parametrize("kind,cin,cout,hw", [("", 8, 8, 32), ("", 32, 32, 8), ("up", 16, 16, 32)])
def test_repeat_launches_bit_identical(kind, cin, cout, hw):
    F_ = 5
    x, w, b, dy = _operands(cin, cout, hw, F_, hw // 2 if kind == "up" else hw)
    a = _launch(x, dy, w, 128, 512, kind=kind)
    c = _launch(x, dy, w, 128, 512, kind=kind)
    for u, v in zip(a, c):
        assert torch.equal(u, v)
