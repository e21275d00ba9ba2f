"""Addressing of the split forward / data-gradient kernels' prefetch
(csrc/conv_split.hip, paig_conv2d_fwd*): the staging loads go through buffer
descriptors of one tile's frames, with out-of-range offsets for idle lanes,
halo rows and channel tails, the per-unit addressing is formed once per block,
and the bias, weight header and weight image are loaded at kernel entry.

Every operand here is a view inside a larger allocation, with a frame stride
of C x H x W + 68 floats and 132 floats at both ends, and everything around
the frames is NaN (0xFF for the pool's window codes): a halo row, channel tail
or frame tail read from a neighbour makes the output non-finite, and after the
launch everything around the output frames must still be NaN.  Launches are
capped at two persistent blocks (paig_debug_fwd_block_cap), so every block
walks several tiles and issues the prefetch past its last one, and the frame
counts are odd (the last multi-frame tile is short of frames).  Results are
compared with the float64 references of tests/test_gpu_persistent.py at its
bars (tests/test_gpu_kernels.py's SPLIT_TOL); with and without
paig_conv_wprep's weight images the outputs are bit-identical.

The C ABI's grouped view (in_grp, in_gs) groups FRAMES (frame f lies at
(f / grp) * fs + (f % grp) * gs); the grouped cases take the frames of a
group from two allocations.  The pool-folding data gradient is instantiated
for the UNet's c4 alone: (32, 32, 32) is the smallest shape on that path."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err
from test_gpu_kernels import DEV, SPLIT_TOL, L, p, st
from test_gpu_persistent import TOL, TOL_G, _pool_fold_ref, _pooled_forward, _up64

pytestmark = pytest.mark.gpu

NAN = float("nan")
GAP, END = 68, 132   # floats between frames / at both ends (multiples of 4: 16-byte aligned frames)
CGAP, CEND = 72, 136   # bytes, for the window codes (read as 8-byte words)
assert SPLIT_TOL[128] == (TOL[128], TOL_G[128]) and SPLIT_TOL[256] == (TOL[256], TOL_G[256])


def _frames(hw):
    return 5 if hw < 16 else 3


def _poisoned(t, fill=None):
    """t [F, ...] as a view with frame stride numel + GAP inside a NaN-filled
    allocation; returns (allocation, view, frame stride)."""
    F_, n = t.shape[0], t[0].numel()
    fs = n + GAP
    buf = torch.full((END + F_ * fs + END,), NAN, device=DEV)
    v = buf[END:END + F_ * fs].view(F_, fs)[:, :n].view(t.shape)
    v.copy_(t)
    return buf, v, fs


def _out(shape, init=NAN):
    buf, v, fs = _poisoned(torch.full(shape, init, device=DEV))
    return buf, v, fs


def _gaps_untouched(buf, v, fs):
    """Nothing outside the view's frames was written (all still NaN)."""
    F_, n = v.shape[0], v[0].numel()
    body = buf[END:END + F_ * fs].view(F_, fs)
    return bool(torch.isnan(buf[:END]).all() and torch.isnan(buf[END + F_ * fs:]).all()
                and torch.isnan(body[:, n:]).all())


def _wprep(w, a, c, ks, dg):
    n = int(L().paig_conv_wprep_size(a, c, ks))
    buf = torch.empty(n, dtype=torch.int16, device=DEV)
    L().paig_conv_wprep(1, (ctypes.c_void_p * 1)(p(w)), (ctypes.c_int * 1)(a), (ctypes.c_int * 1)(c),
                        (ctypes.c_int * 1)(ks), (ctypes.c_int * 1)(dg), (ctypes.c_void_p * 1)(p(buf)), st())
    return buf


def _capped(run, w, a, c, dg, mode, ks=3):
    """run(wprep pointer) under a two-block cap, without and with the weight
    images: bit-identical (f16 split; the bf16 mode takes no image)."""
    L().paig_debug_fwd_block_cap(2)
    try:
        got = run(None)
        if mode == 128:
            img = _wprep(w, a, c, ks, dg)
            again = run(p(img))
            torch.cuda.synchronize()
            for u, v in zip(got, again):
                assert torch.equal(u, v), "weight images change the result"
        torch.cuda.synchronize()
    finally:
        L().paig_debug_fwd_block_cap(0)
    return got


def _data(cin, cout, hw, hin=None, ks=3):
    F_ = _frames(hw)
    hin = hin or hw
    torch.manual_seed(cin * 131 + cout * 7 + hw)
    x = torch.relu(torch.randn(F_, cin, hin, hin, device=DEV))
    w = torch.randn(cout, cin, ks, ks, device=DEV) * (0.6 / cin ** 0.5)
    b = torch.randn(cout, device=DEV) * 0.1
    dy = torch.randn(F_, cout, hw, hw, device=DEV)
    return F_, x, w, b, dy


def _conv64(x, w, b):
    return F.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), padding=w.shape[-1] // 2)


@pytest.mark.parametrize("mode", [128, 256])
@pytest.mark.parametrize("cin,cout,hw", [(8, 8, 32), (16, 32, 8), (3, 8, 32)])
def test_plain_forward(cin, cout, hw, mode):
    """Row tiles, multi-frame tiles with a short last tile, and the channel
    tail (3 of 8 channels; without an image: the in-kernel weight staging)."""
    F_, x, w, b, _ = _data(cin, cout, hw)
    bx, vx, xfs = _poisoned(x)

    def run(wp):
        bo, vo, ofs = _out((F_, cout, hw, hw))
        L().paig_conv2d_fwd_pw(p(vx), xfs, 0, 0, p(vo), ofs, None, 0, p(w), p(b), F_, cin, cout, hw, hw, 3, 1 | mode,
                               None, 0, None, 0, wp, st())
        torch.cuda.synchronize()
        assert _gaps_untouched(bo, vo, ofs), "wrote outside the output frames"
        return (vo.contiguous(),)
    out, = _capped(run, w, cin, cout, 0, mode)
    assert torch.isfinite(out).all()
    assert rel_err(out, torch.relu(_conv64(x, w, b))) <= TOL[mode]


@pytest.mark.parametrize("mode", [128, 256])
@pytest.mark.parametrize("cin,cout,hw", [(24, 8, 32), (32, 16, 16)])
def test_grouped_input(cin, cout, hw, mode):
    """A grouped view (grp = 2): even frames in one allocation, odd frames in
    another, each poisoned around its frames."""
    F_, x, w, b, _ = _data(cin, cout, hw)
    ba, va, fs = _poisoned(x[0::2])
    bb, vb, fs_b = _poisoned(x[1::2].repeat(2, 1, 1, 1)[:va.shape[0]])   # the same frame count: the same stride
    assert fs == fs_b and (vb.data_ptr() - va.data_ptr()) % 4 == 0
    gs = (vb.data_ptr() - va.data_ptr()) // 4

    def run(wp):
        bo, vo, ofs = _out((F_, cout, hw, hw))
        L().paig_conv2d_fwd_pw(p(va), fs, 2, gs, p(vo), ofs, None, 0, p(w), p(b), F_, cin, cout, hw, hw, 3, 1 | mode,
                               None, 0, None, 0, wp, st())
        torch.cuda.synchronize()
        assert _gaps_untouched(bo, vo, ofs), "wrote outside the output frames"
        return (vo.contiguous(),)
    out, = _capped(run, w, cin, cout, 0, mode)
    assert torch.isfinite(out).all()
    assert rel_err(out, torch.relu(_conv64(x, w, b))) <= TOL[mode]


@pytest.mark.parametrize("mode", [128, 256])
@pytest.mark.parametrize("cin,cout,hw", [(32, 16, 16), (16, 16, 32), (32, 16, 18), (16, 16, 36)])
def test_fused_upsample(cin, cout, hw, mode):
    """The half-resolution window through the tile descriptor (3bp's 36 / 18:
    odd tile heights)."""
    hs = hw // 2
    F_, xs, w, b, _ = _data(cin, cout, hw, hin=hs)
    bx, vx, xfs = _poisoned(xs)

    def run(wp):
        bo, vo, ofs = _out((F_, cout, hw, hw))
        L().paig_conv2d_fwd_pw(p(vx), xfs, 0, 0, p(vo), ofs, None, 0, p(w), p(b), F_, cin, cout, hw, hw, 3, 32 | mode,
                               None, 0, None, 0, wp, st())
        torch.cuda.synchronize()
        assert _gaps_untouched(bo, vo, ofs), "wrote outside the output frames"
        return (vo.contiguous(),)
    out, = _capped(run, w, cin, cout, 0, mode)
    assert torch.isfinite(out).all()
    ref = F.conv2d(_up64(xs, hw), w.double().cpu(), b.double().cpu(), padding=1)
    assert rel_err(out, ref) <= TOL[mode]


@pytest.mark.parametrize("mode", [128, 256])
@pytest.mark.parametrize("cin,cout,hw", [(8, 8, 32), (16, 16, 16)])
def test_fused_pool_with_codes(cin, cout, hw, mode):
    assert L().paig_conv2d_mfma_supported(0, cin, cout, hw, hw, 3, mode | 64) == 1
    F_, x, w, b, _ = _data(cin, cout, hw)
    hp = hw // 2
    cfs = -(-cout // 8) * 8 * hp * hp
    cs = cfs + CGAP
    bx, vx, xfs = _poisoned(x)

    def run(wp):
        bo, vo, ofs = _out((F_, cout, hw, hw))
        bp, vp, pfs = _out((F_, cout, hp, hp))
        bc = torch.full((CEND + F_ * cs + CEND,), 255, dtype=torch.uint8, device=DEV)
        L().paig_conv2d_fwd_pwc(p(vx), xfs, 0, 0, p(vo), ofs, None, 0, p(w), p(b), F_, cin, cout, hw, hw, 3,
                                1 | 64 | mode, None, 0, p(vp), pfs, bc.data_ptr() + CEND, cs, wp, st())
        torch.cuda.synchronize()
        assert _gaps_untouched(bo, vo, ofs), "wrote outside the output frames"
        assert _gaps_untouched(bp, vp, pfs), "wrote outside the pooled frames"
        body = bc[CEND:CEND + F_ * cs].view(F_, cs)
        assert bool((bc[:CEND] == 255).all() and (bc[CEND + F_ * cs:] == 255).all() and (body[:, cfs:] == 255).all()), \
            "wrote outside the window codes"
        return vo.contiguous(), vp.contiguous(), body[:, :cfs].contiguous().view(-1)
    y, pool, code = _capped(run, w, cin, cout, 0, mode)
    assert torch.isfinite(y).all()
    assert rel_err(y, torch.relu(_conv64(x, w, b))) <= TOL[mode]
    # the pooled values and window codes of the GPU's own output, bit for bit
    rp = torch.empty_like(pool)
    rc = torch.zeros_like(code)
    L().paig_maxpool2_fwd_codes(p(y), cout * hw * hw, p(rp), cout * hp * hp, p(rc), cfs, F_, cout, hw, hw, st())
    torch.cuda.synchronize()
    assert torch.equal(pool, rp)
    assert torch.equal(code, rc)


@pytest.mark.parametrize("mode", [128, 256])
@pytest.mark.parametrize("cin,cout,hw", [(8, 8, 32), (16, 16, 16)])
def test_dgrad_mask_accumulate(cin, cout, hw, mode):
    """The gradient, the ReLU' mask (prefetched through its own descriptor)
    and the accumulated output, each a poisoned view."""
    assert L().paig_conv2d_mfma_supported(0, cout, cin, hw, hw, 3, 8 | mode) == 1
    F_, x, w, _, dy = _data(cin, cout, hw)
    bd, vd, dfs = _poisoned(dy)
    ba, va, afs = _poisoned(x)

    def run(wp):
        bo, vo, ofs = _out((F_, cin, hw, hw), 0.5)
        L().paig_conv2d_fwd_pw(p(vd), dfs, 0, 0, p(vo), ofs, p(va), afs, p(w), None, F_, cout, cin, hw, hw, 3,
                               8 | 4 | 2 | mode, None, 0, None, 0, wp, st())
        torch.cuda.synchronize()
        assert _gaps_untouched(bo, vo, ofs), "wrote outside dx's frames"
        return (vo.contiguous(),)
    dx, = _capped(run, w, cout, cin, 1, mode)
    assert torch.isfinite(dx).all()
    rdx = (torch.nn.grad.conv2d_input(x.shape, w.double().cpu(), dy.double().cpu(), padding=1) + 0.5) * (x.cpu() > 0)
    assert rel_err(dx, rdx) <= TOL_G[mode]


def test_dgrad_pool_fold():
    """The pooled gradient and the window codes through descriptors of their
    own (the codes' with element size 1)."""
    cin, cout, hw, mode = 32, 32, 32, 128
    assert L().paig_conv2d_mfma_supported(0, cout, cin, hw, hw, 3, 8 | 64 | mode) == 1
    F_, x, w, b, gy = _data(cin, cout, hw)
    hp = hw // 2
    gp = torch.randn(F_, cout, hp, hp, device=DEV)
    y, code, cfs, _ = _pooled_forward(x, w, b, mode)
    cs = cfs + CGAP
    bc = torch.full((CEND + F_ * cs + CEND,), 255, dtype=torch.uint8, device=DEV)
    bc[CEND:CEND + F_ * cs].view(F_, cs)[:, :cfs].copy_(code.view(F_, cfs))
    bg, vg, gfs = _poisoned(gy)
    bp, vp, pfs = _poisoned(gp)
    ba, va, afs = _poisoned(x)

    def run(wp):
        bo, vo, ofs = _out((F_, cin, hw, hw))
        L().paig_conv2d_fwd_pwc(p(vg), gfs, 0, 0, p(vo), ofs, p(va), afs, p(w), None, F_, cout, cin, hw, hw, 3,
                                8 | 64 | 2 | mode, None, 0, p(vp), pfs, bc.data_ptr() + CEND, cs, wp, st())
        torch.cuda.synchronize()
        assert _gaps_untouched(bo, vo, ofs), "wrote outside dx's frames"
        return (vo.contiguous(),)
    dx, = _capped(run, w, cout, cin, 1, mode)
    assert torch.isfinite(dx).all()
    rdx, _, _ = _pool_fold_ref(x, w, y, gy, gp)
    assert rel_err(dx, rdx) <= TOL_G[mode]


def test_dgrad_upsample_transpose():
    """UPT (64, 32, 32): the source's ReLU' input through a descriptor of the
    frame's half-resolution planes."""
    cin, cout, hw, mode = 64, 32, 32, 128
    assert L().paig_conv2d_mfma_supported(0, cout, cin, hw, hw, 3, 8 | mode | 512) == 1
    hs = hw // 2
    F_, xs, w, _, dy = _data(cin, cout, hw, hin=hs)
    bd, vd, dfs = _poisoned(dy)
    ba, va, afs = _poisoned(xs)

    def run(wp):
        bo, vo, ofs = _out((F_, cin, hs, hs))
        L().paig_conv2d_fwd_pw(p(vd), dfs, 0, 0, p(vo), ofs, p(va), afs, p(w), None, F_, cout, cin, hw, hw, 3,
                               8 | mode | 512 | 2, None, 0, None, 0, wp, st())
        torch.cuda.synchronize()
        assert _gaps_untouched(bo, vo, ofs), "wrote outside the source gradient's frames"
        return (vo.contiguous(),)
    got, = _capped(run, w, cout, cin, 1, mode)
    assert torch.isfinite(got).all()
    xr = xs.double().cpu().requires_grad_(True)
    F.conv2d(F.interpolate(xr, size=(hw, hw), mode="bilinear", align_corners=False), w.double().cpu(),
             padding=1).backward(dy.double().cpu())
    assert rel_err(got, xr.grad * (xs.cpu() > 0)) <= TOL_G[mode]


def test_tile_extent_past_2g_is_rejected():
    """Two-frame tiles (8 x 8) with a frame stride that puts one tile's extent
    past 2^31 bytes: the launcher returns the error code and launches nothing.
    One real frame: no launch of this call could touch a second one."""
    from paig_reproduction_amd._lib import PaigError
    cin, cout, hw = 16, 32, 8
    x = torch.randn(1, cin, hw, hw, device=DEV)
    w = torch.randn(cout, cin, 3, 3, device=DEV)
    b = torch.randn(cout, device=DEV)
    out = torch.full((1, cout, hw, hw), NAN, device=DEV)
    with pytest.raises(PaigError, match="32-bit byte offsets"):
        L().paig_conv2d_fwd(p(x), 1 << 29, 0, 0, p(out), cout * hw * hw, None, 0, p(w), p(b), 1, cin, cout, hw, hw, 3,
                            1 | 128, st())
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
