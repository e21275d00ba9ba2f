"""Slab rows of the fused layer backward in accumulator order
(paig_conv2d_bwd flags & 1024, csrc/conv_bwd.hip put_w) and the reduction that
permutes them (paig_slab_reduce_multi_frag, csrc/unet_ops.hip).

Each case calls paig_conv2d_bwd twice on the same random inputs, once with the
default [Cout*Cin*9 | Cout] rows and once with the flag, every slab filled
with NaN beforehand (a padding or unwritten element that reaches the result
fails the case), and asserts

* dx: torch.equal (the layout does not touch the data gradient);
* dW, db of the flagged rows through paig_slab_reduce_multi_frag against the
  default rows through paig_slab_reduce_multi: torch.equal.  That is the
  reduction the training step runs, and the one whose row order and LDS tree
  the new entry point keeps;
* the same against the default rows through paig_slab_reduce: torch.equal
  with at most two rows.  With more rows paig_slab_reduce itself adds in
  another order than paig_slab_reduce_multi (4 row strides and a 4-way
  combine, against 128 row lanes and a binary tree), so the two sums of the
  SAME rows already differ in the last bits.  There the bound is the one
  fp32 summation gives two orders of the same n terms: each is within
  (n - 1) 2^-24 sum_b |row_b| of the exact sum, so they are within twice that
  of each other, element by element.

Shapes: the 8 x 8 levels with multi-frame tiles, the 16 x 16 levels plain,
with the upsample fold and with the pool fold, a Cin that is no multiple of
16 (padded columns) and one with a tail N-tile; F = 3 and 5 (odd: a partial
multi-frame tile); nblk_max = 2 (several tiles per block) and 512 (one tile
per block, several rows); split and bf16 arithmetic."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
XMAX_SLOTS = 2048
# (Cin, Cout, H, kind): kind "up" = fused-upsample input, "pool" = pool fold
SHAPES = [(16, 32, 8, ""), (32, 32, 8, ""), (8, 16, 16, ""), (32, 16, 16, "up"), (16, 16, 16, "pool"),
          (24, 8, 32, ""), (8, 8, 32, "")]


def L():
    from paig_reproduction_amd._lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def _arr(ct, *v):
    return (ct * len(v))(*v)


def _operands(cin, cout, hw, kind, F_, mode):
    """Random operands of one layer and what its forward leaves for the
    backward (the X maxima; pool fold: the pooled gradient and window codes)."""
    hx = hw // 2 if kind == "up" else hw
    x = torch.relu(torch.randn(F_, cin, hx, hx, device=DEV))
    w = torch.randn(cout, cin, 3, 3, device=DEV) * 0.2
    b = torch.randn(cout, device=DEV) * 0.1
    dy = torch.randn(F_, cout, hw, hw, device=DEV)
    xmax = torch.zeros(XMAX_SLOTS, device=DEV)
    y = torch.empty(F_, cout, hw, hw, device=DEV)
    xm, xn = (p(xmax), XMAX_SLOTS) if mode == 128 else (None, 0)
    hp = hw // 2
    gp = code = None
    cfs = 0
    if kind == "pool":
        gp = torch.randn(F_, cout, hp, hp, device=DEV)
        pool = torch.empty(F_, cout, hp, hp, device=DEV)
        cfs = -(-cout // 8) * 8 * hp * hp
        code = torch.empty(F_ * cfs, dtype=torch.uint8, device=DEV)
        L().paig_conv2d_fwd_pwc(p(x), cin * hw * hw, 0, 0, p(y), cout * hw * hw, None, 0, p(w), p(b), F_, cin, cout,
                                hw, hw, 3, 1 | 64 | mode, xm, xn, p(pool), cout * hp * hp, p(code), cfs, None, st())
    else:
        L().paig_conv2d_fwd_ex(p(x), cin * hx * hx, 0, 0, p(y), cout * hw * hw, None, 0, p(w), p(b), F_, cin, cout,
                               hw, hw, 3, mode | (32 if kind == "up" else 0), xm, xn, st())
    return dict(x=x, w=w, dy=dy, xmax=xmax, xm=xm, xn=xn, gp=gp, code=code, cfs=cfs, hx=hx, hp=hp)   # (xmax: keeps xm alive)


def _bwd(o, cin, cout, hw, kind, F_, mode, nmax, row_flag):
    """One launch into a NaN-filled slab: (dx, slab, rows, row length)."""
    flags = mode | 2 | {"": 0, "up": 32, "pool": 64}[kind] | row_flag
    slen = int(L().paig_conv2d_bwd_slab_len(cin, cout, 3, row_flag))
    slab = torch.full((nmax * slen,), float("nan"), device=DEV)
    dx = torch.full((F_, cin, o["hx"], o["hx"]), float("nan"), device=DEV)
    nb = ctypes.c_int(0)
    xfs = cin * o["hx"] * o["hx"]
    L().paig_conv2d_bwd(p(o["x"]), xfs, 0, 0, p(o["dy"]), cout * hw * hw, p(dx), xfs, p(o["x"]), xfs, p(o["w"]),
                        p(slab), nmax, ctypes.byref(nb), F_, cin, cout, hw, hw, 3, flags, o["xm"], o["xn"],
                        p(o["gp"]), cout * o["hp"] * o["hp"], p(o["code"]), o["cfs"], None, st())
    return dx, slab, nb.value, slen


def _reduce_multi(slab, nb, slen, n_out, cin=0, cout=0, dst=None, accumulate=0):
    g = torch.empty(n_out, device=DEV) if dst is None else dst
    P, I = ctypes.c_void_p, ctypes.c_int
    if cin:
        L().paig_slab_reduce_multi_frag(1, _arr(P, p(slab)), _arr(I, nb), _arr(I, slen), _arr(P, p(g)), _arr(I, cin),
                                        _arr(I, cout), accumulate, st())
    else:
        L().paig_slab_reduce_multi(1, _arr(P, p(slab)), _arr(I, nb), _arr(I, slen), _arr(P, p(g)), accumulate, st())
    return g


@pytest.mark.parametrize("mode", [128, 256], ids=["split", "bf16"])
@pytest.mark.parametrize("cin,cout,hw,kind", SHAPES)
def test_accumulator_order_rows_same_bits(cin, cout, hw, kind, mode):
    assert L().paig_conv2d_bwd_supported(cin, cout, hw, hw, 3, mode | {"": 0, "up": 32, "pool": 64}[kind]) == 1
    n = cout * cin * 9 + cout
    assert int(L().paig_conv2d_bwd_slab_len(cin, cout, 3, 0)) == n
    nfrag = -(-cout // 16) * -(-(9 * cin // 4) // 4) * 256 + cout
    assert int(L().paig_conv2d_bwd_slab_len(cin, cout, 3, 1024)) == nfrag
    for F_ in (3, 5):
        torch.manual_seed(cin * 1000 + cout * 10 + hw + F_ + mode)
        o = _operands(cin, cout, hw, kind, F_, mode)
        for nmax in (2, 512):
            dx0, slab0, nb0, len0 = _bwd(o, cin, cout, hw, kind, F_, mode, nmax, 0)
            dx1, slab1, nb1, len1 = _bwd(o, cin, cout, hw, kind, F_, mode, nmax, 1024)
            assert nb0 == nb1 and 1 <= nb0 <= nmax and len0 == n and len1 == nfrag
            g_multi = _reduce_multi(slab0, nb0, len0, n)
            g_frag = _reduce_multi(slab1, nb1, len1, n, cin, cout)
            g_plain = torch.empty(n, device=DEV)
            L().paig_slab_reduce(p(slab0), nb0, n, n, p(g_plain), 0, st())
            torch.cuda.synchronize()
            case = (F_, nmax, nb0)
            assert torch.isfinite(dx0).all() and torch.equal(dx0, dx1), case
            assert torch.isfinite(g_multi).all(), case
            assert torch.equal(g_frag[:n - cout], g_multi[:n - cout]), ("dW", case)
            assert torch.equal(g_frag[n - cout:], g_multi[n - cout:]), ("db", case)
            if nb0 <= 2:
                assert torch.equal(g_frag, g_plain), ("paig_slab_reduce", case)
            else:
                rows = slab0[:nb0 * n].view(nb0, n).double()
                bound = 2 * (nb0 - 1) * 2.0 ** -24 * rows.abs().sum(0)
                err = (g_frag.double() - g_plain.double()).abs()
                print(f"{case}: max |frag - paig_slab_reduce| / bound = {(err / bound.clamp_min(1e-300)).max():.3f}")
                assert (err <= bound).all(), ("paig_slab_reduce", case)


def test_accumulator_order_shape_without_it_is_refused():
    """3bp's plain 8 -> 8 at 36 x 36 (split) does not compile the second store
    path (sbwd_fragrows): the query says so and the launch is an error, not
    rows in another layout than asked for."""
    from paig_reproduction_amd._lib import PaigError
    assert L().paig_conv2d_bwd_supported(8, 8, 36, 36, 3, 128) == 1
    assert L().paig_conv2d_bwd_supported(8, 8, 36, 36, 3, 128 | 1024) == 0
    assert L().paig_conv2d_bwd_supported(8, 8, 36, 36, 3, 128 | 64 | 1024) == 1
    torch.manual_seed(3)
    o = _operands(8, 8, 36, "", 1, 128)
    with pytest.raises(PaigError):
        _bwd(o, 8, 8, 36, "", 1, 128, 4, 1024)


def test_accumulator_order_reduce_scalar_path_and_accumulate():
    """A destination that is not 16-byte aligned takes the scalar path for
    plain and permuted rows alike, and accumulate adds to what is there: the
    same bits as the plain rows in both."""
    cin, cout, hw, F_, mode = 24, 8, 32, 3, 128
    torch.manual_seed(5)
    o = _operands(cin, cout, hw, "", F_, mode)
    n = cout * cin * 9 + cout
    _, slab0, nb0, len0 = _bwd(o, cin, cout, hw, "", F_, mode, 512, 0)
    _, slab1, nb1, len1 = _bwd(o, cin, cout, hw, "", F_, mode, 512, 1024)
    assert nb0 == nb1 > 2
    for accumulate in (0, 1):
        for off in (0, 1):   # floats: 0 = aligned (vector path), 1 = scalar path
            init = torch.randn(n + 4, device=DEV)
            a, c = init.clone(), init.clone()
            _reduce_multi(slab0, nb0, len0, n, dst=a[off:off + n], accumulate=accumulate)
            _reduce_multi(slab1, nb1, len1, n, cin, cout, dst=c[off:off + n], accumulate=accumulate)
            torch.cuda.synchronize()
            assert torch.isfinite(a).all() and torch.equal(a, c), (accumulate, off)
