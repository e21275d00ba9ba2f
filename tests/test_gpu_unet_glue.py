"""The U-Net glue kernels of csrc/unet_ops.hip alone, through the C ABI, in every
form their entry points launch, against tests/unet_glue_ref.py (which
tests/test_unet_glue_ref_cpu.py holds against aten): paig_maxpool2_fwd,
paig_maxpool2_fwd_codes, paig_maxpool2_bwd_relu, paig_upsample2_fwd,
paig_upsample2_bwd; and three small companions without a direct test:
paig_axpby, paig_relu_mask (csrc/misc.hip) and the single-task paig_slab_reduce.

Each case's id names the form it is meant to reach.  The forms are chosen on the
host by these conditions, quoted from unet_ops.hip (tests/test_unet_glue_ref_cpu.py
fails when a quotation is no longer in the source, so a changed dispatch shows):

  maxpool2_fwd, vector (maxpool_fwd_v_k) if
    ``H % 2 == 0 && W % 4 == 0 && x_fs % 4 == 0 && y_fs % 2 == 0 && (long long)F * C * H * W < (1ll << 31) &&
      (uintptr_t)x % 16 == 0 && (uintptr_t)y % 8 == 0``
  else scalar (maxpool_fwd_k<int>).
  maxpool2_bwd_relu, vector (maxpool_bwd_relu_v_k) if
    ``H % 2 == 0 && W % 4 == 0 && x_fs % 4 == 0 && dx_fs % 4 == 0 && dy_fs % 2 == 0 &&
      (long long)F * C * H * W < (1ll << 31) && (uintptr_t)x % 16 == 0 && (uintptr_t)dx % 16 == 0 &&
      (uintptr_t)dy % 8 == 0``
  else scalar (maxpool_bwd_relu_k<int>).
  maxpool2_fwd_codes, one kernel, refused unless
    ``H % 2 == 0 && W % 2 == 0 && code && code_fs >= (long long)(C + 7) / 8 * 8 * (H / 2) * (W / 2) &&
                   (long long)F * C * H * W < (1ll << 31)``
  upsample2_fwd: one kernel (upsample_fwd_k<int>).
  upsample2_bwd, refused unless ``Ho == 2 * Hs && Wo == 2 * Ws``; vector (upsample_bwd_v_k) if
    ``Ws % 2 == 0 && Wo % 4 == 0 && du_fs % 4 == 0 && ds_fs % 2 == 0 && (!relu_mask || s_fs % 2 == 0) &&
      (long long)F * C * Ho * Wo < (1ll << 31) && (uintptr_t)du % 16 == 0 && (uintptr_t)ds % 8 == 0 &&
      (!relu_mask || (uintptr_t)s % 8 == 0)``
  else scalar (upsample_bwd_k<int>); inside the vector kernel, P = Ws / 2, the edge
  columns come by lane shuffle under ``if (64 % P == 0) {`` and by two scalar
  loads otherwise (P not a divisor of 64, or P > 64).
  Grids: ``if (g > 8192) g = 8192;`` blocks of 256 threads, so past 2,097,152 work
  items a thread takes a second trip; paig_relu_mask's is
  ``n / 256 + 1 < 4096 ? n / 256 + 1 : 4096``.

The <long long> instantiations of the scalar kernels are launched only when
``n + 8192LL * 256 < (1ll << 31)`` fails: at least 2^31 elements, 8 GB per
buffer.  No test here reaches them.

Every output is NaN before the call (code bytes: 0xA5), lies between sentinels,
and where its frame stride exceeds the frame the gap is padding: sentinels and
padding must be unchanged afterwards.  Input padding is NaN too.

Bounds.  The pool selects values and its backward adds once per element, so
both are compared bit for bit with the fp32 reference.  The upsample is held
to the normwise 1e-6 of test_gpu_kernels.py::test_pool_upsample and, per
element, to |got - want| <= n 2^-23 sum |w| |v|: the rounding bound n 2^-24 of
an n-term dot product (n = 4 taps forward, 16 backward; the weights 1/4, 3/4,
1 are exact) with a factor 2 of margin; the worst ratio is printed as
GLUE_ERR <kernel> <case> <ratio>."""
import pytest
import torch

import unet_glue_ref as R
from dense_gpu import DEV, Guard, L, dev, gen, ptr, refused, rnd, same_bits, st
from helpers import rel_err

pytestmark = pytest.mark.gpu
NAN = float("nan")
FILL = 0xA5
_fc = lambda c: f"F{c[0]}C{c[1]}"   # noqa: E731
_name = lambda c: c[0]              # noqa: E731


# ----------------------------------------------------------------- plumbing --
def put(t, off=0, pad=0):
    """Device copy of the CPU frames t [F][...] at frame stride numel/F + pad,
    off floats into its buffer, everything around the frames NaN -> (view, fs)"""
    F, n = t.shape[0], t[0].numel()
    fs = n + pad
    buf = torch.full((off + F * fs + 4,), NAN, device=DEV)
    v = buf[off:off + F * fs].view(F, fs)
    v[:, :n].copy_(t.reshape(F, n).float())
    return v, fs


def out(G, F, n, off=0, pad=0, init=None):
    """A guarded NaN output of F frames of n floats at stride n + pad -> (view, fs)"""
    v = G.out(F, n + pad, off=off)
    if init is not None:
        v[:, :n].copy_(init.reshape(F, n))
    return v, n + pad


def take(G, v, n, shape):
    """after the call: sentinels and padding intact -> the frames on the CPU"""
    G.check()
    assert bool(torch.isnan(v[:, n:]).all()), "the padding between frames was written"
    return v[:, :n].cpu().reshape(shape)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits32(got, want, what):
    """bit for bit, -0.0 and 0.0 apart; an unwritten (NaN) element differs"""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {got.numel()} elements differ in bits"


def same_with_nans(got, want, what):
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN masks differ"
    same_bits32(torch.nan_to_num(got), torch.nan_to_num(want), what)


def aligned(v, k):
    return v.data_ptr() % k == 0


# --------------------------------------------------------------------- pool --
# layout: (x offset, x padding, y offset, y padding) in floats; dx lies as x, dy as y
CONTIG, SLICE, OFF1 = (0, 0, 0, 0), (4, 4, 4, 2), (1, 0, 1, 0)
POOL_CASES = [
    ("vector-2x4", 2, 4, CONTIG, "vector"),
    ("vector-4x8", 4, 8, CONTIG, "vector"),
    ("vector-6x12", 6, 12, CONTIG, "vector"),
    ("vector-channel-slice-6x12", 6, 12, SLICE, "vector"),
    ("scalar-W%4-2x2", 2, 2, CONTIG, "scalar"),
    ("scalar-W%4-6x6", 6, 6, CONTIG, "scalar"),
    ("scalar-W%4-18x18", 18, 18, CONTIG, "scalar"),
    ("scalar-odd-H-odd-W-5x7", 5, 7, CONTIG, "scalar"),
    ("scalar-odd-H-5x8", 5, 8, CONTIG, "scalar"),
    ("scalar-x-one-float-in-4x8", 4, 8, (1, 0, 0, 0), "scalar"),
    ("scalar-y-one-float-in-4x8", 4, 8, (0, 0, 1, 0), "scalar"),
    ("scalar-x_fs-odd-4x8", 4, 8, (0, 1, 0, 0), "scalar"),
    ("scalar-y_fs-odd-4x8", 4, 8, (0, 0, 0, 1), "scalar"),
]
assert {c[1:3] for c in POOL_CASES} == set(R.POOL_HW)


def _pool_fwd(x, lay, form):
    F, C, H, W = x.shape
    n = C * (H // 2) * (W // 2)
    G = Guard()
    xd, x_fs = put(x, lay[0], lay[1])
    y, y_fs = out(G, F, n, lay[2], lay[3])
    vec = (H % 2 == 0 and W % 4 == 0 and x_fs % 4 == 0 and y_fs % 2 == 0 and aligned(xd, 16) and aligned(y, 8))
    assert vec == (form == "vector"), "the case does not reach the form its id names"
    L().paig_maxpool2_fwd(ptr(xd), x_fs, ptr(y), y_fs, F, C, H, W, st())
    return take(G, y, n, (F, C, H // 2, W // 2))


def _pool_bwd(x, dy, dx0, lay, form):
    F, C, H, W = x.shape
    n, no = C * H * W, C * (H // 2) * (W // 2)
    G = Guard()
    xd, x_fs = put(x, lay[0], lay[1])
    dyd, dy_fs = put(dy, lay[2], lay[3])
    dx, dx_fs = out(G, F, n, lay[0], lay[1], init=dx0)
    vec = (H % 2 == 0 and W % 4 == 0 and x_fs % 4 == 0 and dx_fs % 4 == 0 and dy_fs % 2 == 0 and aligned(xd, 16) and
           aligned(dx, 16) and aligned(dyd, 8))
    assert vec == (form == "vector"), "the case does not reach the form its id names"
    L().paig_maxpool2_bwd_relu(ptr(xd), x_fs, ptr(dyd), dy_fs, ptr(dx), dx_fs, F, C, H, W, st())
    assert no == dy[0].numel()
    return take(G, dx, n, (F, C, H, W))


def _pool_codes(x, lay, code_pad):
    """-> (pooled, code [F][G][Ho][Wo][8]) at code frame stride minimum + code_pad bytes"""
    F, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    n, nmin = C * Ho * Wo, (C + 7) // 8 * 8 * Ho * Wo
    G = Guard()
    xd, x_fs = put(x, lay[0], lay[1])
    y, y_fs = out(G, F, n, lay[2], lay[3])
    cfs = nmin + code_pad
    cbuf = torch.full((16 + F * cfs + 16,), FILL, dtype=torch.uint8, device=DEV)
    L().paig_maxpool2_fwd_codes(ptr(xd), x_fs, ptr(y), y_fs, cbuf.data_ptr() + 16, cfs, F, C, H, W, st())
    got = take(G, y, n, (F, C, Ho, Wo))
    c = cbuf.cpu()
    assert bool((c[:16] == FILL).all()) and bool((c[-16:] == FILL).all()), "a sentinel beside the codes was written"
    body = c[16:-16].view(F, cfs)
    assert bool((body[:, nmin:] == FILL).all()), "the padding between code frames was written"
    return got, body[:, :nmin].reshape(F, (C + 7) // 8, Ho, Wo, 8)


@pytest.mark.parametrize("fc", R.POOL_FC, ids=_fc)
@pytest.mark.parametrize("case", POOL_CASES, ids=_name)
def test_pool_fwd(case, fc):
    _, H, W, lay, form = case
    for kind, make in (("ties", R.ties), ("gauss", R.gauss), ("nan", R.with_nans)):
        x = make(R.rng(H, W, fc), *fc, H, W)
        want, _ = R.pool_fwd(x)
        same = same_with_nans if kind == "nan" else same_bits32
        got = _pool_fwd(x, lay, form)
        same(got, want, f"pooled, {kind}")
        if form == "vector":
            same(_pool_fwd(x, OFF1, "scalar"), got, f"scalar form against vector form, {kind}")


@pytest.mark.parametrize("fc", R.POOL_FC, ids=_fc)
@pytest.mark.parametrize("case", POOL_CASES, ids=_name)
def test_pool_bwd_relu(case, fc):
    _, H, W, lay, form = case
    for kind, make in (("ties", R.ties), ("gauss", R.gauss)):
        g = R.rng(H, W, fc)
        x = make(g, *fc, H, W)
        dy, dx0 = torch.randn(*fc, H // 2, W // 2, generator=g), torch.randn(*fc, H, W, generator=g)
        want = R.pool_bwd_relu(x, dy, dx0)
        got = _pool_bwd(x, dy, dx0, lay, form)
        same_bits32(got, want, f"dx, {kind}")
        assert bool((bits(got)[x <= 0] == 0).all()), "dx is +0.0 wherever x <= 0"
        if form == "vector":
            same_bits32(_pool_bwd(x, dy, dx0, OFF1, "scalar"), got, f"scalar form against vector form, {kind}")


@pytest.mark.parametrize("fc", R.POOL_FC, ids=_fc)
@pytest.mark.parametrize("layout", [("contiguous-minimal-code_fs", CONTIG, 0), ("channel-slice-code_fs+24", SLICE, 24)],
                         ids=_name)
@pytest.mark.parametrize("hw", R.CODE_HW, ids=lambda c: f"{c[0]}x{c[1]}")
def test_pool_fwd_codes(hw, layout, fc):
    _, lay, code_pad = layout
    for kind, make in (("ties", R.ties), ("gauss", R.gauss), ("nan", R.with_nans)):
        x = make(R.rng(*hw, fc), *fc, *hw)
        got, code = _pool_codes(x, lay, code_pad)
        (same_with_nans if kind == "nan" else same_bits32)(got, R.pool_fwd(x)[0], f"pooled, {kind}")
        C = fc[1]
        assert torch.equal(R.codes_by_channel(code, C), R.codes_by_channel(R.pool_codes(x), C)), f"code bytes, {kind}"


# ----------------------------------------------------------------- upsample --
# layout: (du offset, du padding, ds offset, ds padding, s offset, s padding);
# the forward reads s where the backward does and writes u where du lies
UP_CONTIG, UP_SLICE, UP_OFF1 = (0,) * 6, (4, 4, 4, 2, 4, 2), (1, 0, 0, 0, 0, 0)
UP_CASES = [(f"scalar-odd-Ws-{h}x{w}", h, w, UP_CONTIG, "scalar") for h, w in [(1, 1), (3, 5), (9, 9)]]
UP_CASES += [(f"vector-shuffle-P{w // 2}-{h}x{w}", h, w, UP_CONTIG, "shuffle")
             for h, w in [(1, 2), (2, 4), (3, 8), (5, 16), (2, 64), (2, 128)]]
UP_CASES += [(f"vector-edge-loads-P{w // 2}-{h}x{w}", h, w, UP_CONTIG, "loads") for h, w in [(2, 6), (18, 18), (3, 12)]]
UP_CASES += [
    ("vector-edge-loads-P128-1x256", 1, 256, UP_CONTIG, "loads"),
    ("scalar-du-one-float-in-3x8", 3, 8, (1, 0, 0, 0, 0, 0), "scalar"),
    ("scalar-ds-one-float-in-3x8", 3, 8, (0, 0, 1, 0, 0, 0), "scalar"),
    ("scalar-du_fs+2-3x8", 3, 8, (0, 2, 0, 0, 0, 0), "scalar"),
    ("scalar-with-relu_mask-s-one-float-in-3x8", 3, 8, (0, 0, 0, 0, 1, 0), "scalar if relu_mask"),
    ("vector-edge-loads-channel-slice-18x18", 18, 18, UP_SLICE, "loads"),
]
assert {c[1:3] for c in UP_CASES} == set(R.UP_HW)
_worst = {}


def _bounded(kernel, case, got, want, asum, taps):
    """the normwise 1e-6 and the per-element n 2^-23 sum |w| |v|"""
    g = got.double()
    assert bool(torch.isfinite(g).all()), f"{kernel} {case}: an element is unwritten or not finite"
    e = rel_err(g, want)
    err, bound = (g - want).abs(), taps * 2.0 ** -23 * asum
    nz = bound > 0
    ratio = float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
    _worst[kernel] = max(_worst.get(kernel, 0.0), ratio)
    print(f"GLUE_ERR {kernel} {case} {ratio:.4f}   (normwise {e:.2e}, worst of {kernel} so far {_worst[kernel]:.4f})")
    assert e <= 1e-6, f"{kernel} {case}: normwise {e:.3e} > 1e-6"
    assert bool((err[~nz] == 0).all()), f"{kernel} {case}: not exactly zero where every term is zero"
    assert ratio <= 1.0, f"{kernel} {case}: {ratio:.3f} times the per-element bound"


def _up_fwd(s, lay):
    F, C, Hs, Ws = s.shape
    n = C * 4 * Hs * Ws
    G = Guard()
    sd, s_fs = put(s, lay[4], lay[5])
    u, u_fs = out(G, F, n, lay[0], lay[1])
    L().paig_upsample2_fwd(ptr(sd), s_fs, ptr(u), u_fs, F, C, Hs, Ws, 2 * Hs, 2 * Ws, st())
    return take(G, u, n, (F, C, 2 * Hs, 2 * Ws))


def _up_bwd(du, s, relu, lay, form):
    F, C, Hs, Ws = s.shape
    n = C * Hs * Ws
    G = Guard()
    dud, du_fs = put(du, lay[0], lay[1])
    sd, s_fs = put(s, lay[4], lay[5])
    ds, ds_fs = out(G, F, n, lay[2], lay[3])
    vec = (Ws % 2 == 0 and (2 * Ws) % 4 == 0 and du_fs % 4 == 0 and ds_fs % 2 == 0 and (not relu or s_fs % 2 == 0) and
           aligned(dud, 16) and aligned(ds, 8) and (not relu or aligned(sd, 8)))
    P = Ws // 2
    reached = "scalar" if not vec else ("shuffle" if 64 % P == 0 else "loads")
    if form == "scalar if relu_mask":
        form = "scalar" if relu else "shuffle"
    assert reached == form, "the case does not reach the form its id names"
    L().paig_upsample2_bwd(ptr(dud), du_fs, ptr(sd), s_fs, ptr(ds), ds_fs, F, C, Hs, Ws, 2 * Hs, 2 * Ws, relu, st())
    return take(G, ds, n, (F, C, Hs, Ws)), reached


def _check_upsample(name, Hs, Ws, lay, form, fc):
    g = R.rng(Hs, Ws, fc)
    s = R.gauss(g, *fc, Hs, Ws)
    du = torch.randn(*fc, 2 * Hs, 2 * Ws, generator=g)
    key = f"{name}-{_fc(fc)}"
    _bounded("upsample2_fwd", key, _up_fwd(s, lay), *R.up_fwd(s), taps=4)
    for relu in (0, 1):
        got, reached = _up_bwd(du, s, relu, lay, form)
        _bounded("upsample2_bwd", f"{key}-relu{relu}", got, *R.up_bwd(du, s if relu else None), taps=16)
        if relu:
            assert bool((bits(got)[s <= 0] == 0).all()), "relu_mask: ds is exactly +0.0 wherever s <= 0 (-0.0 too)"
        if reached != "scalar":
            other, r2 = _up_bwd(du, s, relu, UP_OFF1, "scalar")
            same_bits32(other, got, f"scalar form against the vector form ({reached}), relu_mask {relu}")


@pytest.mark.parametrize("fc", R.UP_FC, ids=_fc)
@pytest.mark.parametrize("case", UP_CASES, ids=_name)
def test_upsample(case, fc):
    _check_upsample(*case, fc)


def test_upsample_bwd_partial_last_wave():
    """3 x 8 with F = 1, C = 3: 36 work items of the shuffle arm, a last wave of 36 of its 64 lanes"""
    Hs, Ws, fc = R.PARTIAL_WAVE
    assert fc[0] * fc[1] * Hs * (Ws // 2) == 36
    _check_upsample("vector-shuffle-P4-3x8-partial-wave", Hs, Ws, UP_CONTIG, "shuffle", fc)


# ----------------------------------------- second trip of the grid-stride loop --
@pytest.mark.parametrize("case", R.SECOND, ids=_name)
def test_second_trip_of_the_grid_stride_loop(case):
    """C = 2 and the smallest frame of each form, frames enough for 2,097,152 +
    about 1000 work items (nv or n of the entry point): the last thousand are
    the second trip of the first blocks' threads."""
    name, kernel, H, W, per_frame, form = case
    F, C = R.frames_for(per_frame), 2
    lay = CONTIG if kernel.startswith("pool") else UP_CONTIG
    g = R.rng(H, W, (F, C))
    if kernel.startswith("pool"):
        x = R.ties(g, F, C, H, W)
        if kernel == "pool_fwd":
            same_bits32(_pool_fwd(x, lay, form), R.pool_fwd(x)[0], "pooled")
        elif kernel == "pool_codes":
            got, code = _pool_codes(x, lay, 0)
            same_bits32(got, R.pool_fwd(x)[0], "pooled")
            assert torch.equal(R.codes_by_channel(code, C), R.codes_by_channel(R.pool_codes(x), C)), "code bytes"
        else:
            dy, dx0 = torch.randn(F, C, H // 2, W // 2, generator=g), torch.randn(F, C, H, W, generator=g)
            same_bits32(_pool_bwd(x, dy, dx0, lay, form), R.pool_bwd_relu(x, dy, dx0), "dx")
    else:
        s = R.gauss(g, F, C, H, W)
        if kernel == "up_fwd":
            _bounded("upsample2_fwd", name, _up_fwd(s, lay), *R.up_fwd(s), taps=4)
        else:
            du = torch.randn(F, C, 2 * H, 2 * W, generator=g)
            for relu in (0, 1):
                got, _ = _up_bwd(du, s, relu, lay, form)
                _bounded("upsample2_bwd", f"{name}-relu{relu}", got, *R.up_bwd(du, s if relu else None), taps=16)
                if relu:
                    assert bool((bits(got)[s <= 0] == 0).all())


# ---------------------------------------------------------------- refusals --
def _codes_args(C, H, W, code, code_fs, G):
    x = dev(rnd(gen(1), 1, C, H, W))
    y = G.out(1, C, H // 2, W // 2)
    return (ptr(x), C * H * W, ptr(y), C * (H // 2) * (W // 2), code, code_fs, 1, C, H, W, st()), x


@pytest.mark.parametrize("what", ["odd-H", "odd-W", "null-code", "code_fs-one-byte-short"])
def test_pool_fwd_codes_refusals(what):
    C, H, W = 3, 4, 8
    if what == "odd-H":
        H = 5
    if what == "odd-W":
        W = 7
    need = (C + 7) // 8 * 8 * (H // 2) * (W // 2)
    cbuf = torch.full((need + 64,), FILL, dtype=torch.uint8, device=DEV)
    G = Guard()
    args, keep = _codes_args(C, H, W, None if what == "null-code" else cbuf.data_ptr(),
                             need - 1 if what == "code_fs-one-byte-short" else need, G)
    refused(L().paig_maxpool2_fwd_codes, *args)
    G.untouched()
    assert bool((cbuf == FILL).all()), "a refused call wrote code bytes"


@pytest.mark.parametrize("what", ["Ho-not-2Hs", "Wo-not-2Ws"])
def test_upsample_bwd_refusals(what):
    F, C, Hs, Ws = 1, 2, 3, 4
    Ho, Wo = (2 * Hs + 1, 2 * Ws) if what == "Ho-not-2Hs" else (2 * Hs, 2 * Ws + 4)
    g, G = gen(3), Guard()
    du, s = dev(rnd(g, F, C, Ho, Wo)), dev(rnd(g, F, C, Hs, Ws))
    ds = G.out(F, C, Hs, Ws)
    for relu in (0, 1):
        refused(L().paig_upsample2_bwd, ptr(du), C * Ho * Wo, ptr(s), C * Hs * Ws, ptr(ds), C * Hs * Ws, F, C, Hs, Ws,
                Ho, Wo, relu, st())
    G.untouched()


def test_no_frames_is_no_work():
    """F = 0: status 0 and nothing written, all five entry points"""
    C, H, W = 3, 4, 8
    g, G = gen(5), Guard()
    x, dy, s = dev(rnd(g, 1, C, H, W)), dev(rnd(g, 1, C, H // 2, W // 2)), dev(rnd(g, 1, C, H // 2, W // 2))
    y, dx, u, ds = G.out(1, C, H // 2, W // 2), G.out(1, C, H, W), G.out(1, C, H, W), G.out(1, C, H // 2, W // 2)
    cbuf = torch.full((256,), FILL, dtype=torch.uint8, device=DEV)
    n, no = C * H * W, C * (H // 2) * (W // 2)
    Lb = L()
    assert Lb.paig_maxpool2_fwd(ptr(x), n, ptr(y), no, 0, C, H, W, st()) == 0
    assert Lb.paig_maxpool2_fwd_codes(ptr(x), n, ptr(y), no, cbuf.data_ptr(), 256, 0, C, H, W, st()) == 0
    assert Lb.paig_maxpool2_bwd_relu(ptr(x), n, ptr(dy), no, ptr(dx), n, 0, C, H, W, st()) == 0
    assert Lb.paig_upsample2_fwd(ptr(s), no, ptr(u), n, 0, C, H // 2, W // 2, H, W, st()) == 0
    assert Lb.paig_upsample2_bwd(ptr(u), n, ptr(s), no, ptr(ds), no, 0, C, H // 2, W // 2, H, W, 1, st()) == 0
    G.untouched()
    assert bool((cbuf == FILL).all())


# -------------------------------------------------------------- companions --
def _ulps(a, b):
    """distance in units in the last place between two finite fp32 tensors"""
    def order(t):
        i = bits(t).to(torch.int64)
        return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))
    return (order(a) - order(b)).abs()


@pytest.mark.parametrize("ab", [(1.0, 1.0), (0.5, -2.0), (1.0, 0.0)], ids=lambda c: f"a{c[0]}b{c[1]}")
@pytest.mark.parametrize("n", [1, 255, 257, R.TRIP + 1000])
def test_axpby(n, ab):
    """y = a x + b y (flat.py's gradient accumulation).  Each element is the
    fp32 host expression, or at most 1 ulp from it should the compiler contract
    a*x + b*y into an fma; with b = 0, y is not read (NaN before the call) and
    the result a*x + 0 is one rounding however it is compiled: exact."""
    a, b = ab
    g, G = gen(n), Guard()
    x32, y32 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    x, y = dev(x32), G.out(n)
    if b != 0:
        y.copy_(y32)
    L().paig_axpby(ptr(x), ptr(y), n, a, b, st())
    G.check()
    want = a * x32 + b * y32 if b != 0 else a * x32
    got = y.cpu()
    assert want.dtype == torch.float32 and bool(torch.isfinite(got).all())
    d = int(_ulps(got, want).max())
    print(f"GLUE_ERR axpby n{n}-a{a}-b{b} {d} ulp ({'exact' if d == 0 else 'not exact'})")
    assert d <= (0 if b == 0 else 1)
    if b == 0:
        same_bits32(got, a * x32, "a x with b = 0")


@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 1000])
def test_relu_mask(n):
    """d = y > 0 ? d : 0 in place; its grid stops at 4096 blocks"""
    g, G = gen(n), Guard()
    y32, d32 = R.gauss(g, n), torch.randn(n, generator=g)
    if n > 1:
        assert bool((y32 < 0).any()) and bool((bits(y32) == 0).any()) and bool((bits(y32) == -2 ** 31).any())
    else:
        y32[0] = -0.0
    y, d = dev(y32), G.out(n)
    d.copy_(d32)
    L().paig_relu_mask(ptr(y), ptr(d), n, st())
    G.check()
    same_bits32(d.cpu(), torch.where(y32 > 0, d32, torch.zeros(n)), "d")


@pytest.mark.parametrize("accumulate", [0, 1])
def test_slab_reduce(accumulate):
    """out[i] (+)= sum_b slab[b][i], the single-task reduction most conv tests
    reduce with: against the fp64 column sum under test_slab_reduce_multi's
    1e-4 max(1, max |want|); the columns [len, ld) are never read (NaN); two
    runs give the same bits."""
    Lb = L()
    for nblk in (0, 1, 3, 4, 5, 130):
        for ln in (1, 63, 64, 65, 200):
            g = gen(1000 * nblk + ln)
            ld = ln + 3
            slab32 = torch.full((nblk, ld), NAN)
            slab32[:, :ln] = rnd(g, nblk, ln)
            out0 = rnd(g, ln)
            slab = dev(slab32)
            want = slab32[:, :ln].double().sum(0) + (out0.double() if accumulate else 0)
            runs = []
            for _ in range(2):
                G = Guard()
                o = G.out(ln)
                if accumulate:
                    o.copy_(out0)
                Lb.paig_slab_reduce(ptr(slab) if nblk else None, nblk, ld, ln, ptr(o), accumulate, st())
                G.check()
                runs.append(o.cpu())
            what = f"nblk {nblk} len {ln} accumulate {accumulate}"
            assert bool(torch.isfinite(runs[0]).all()), what
            e = float((runs[0].double() - want).abs().max())
            assert e <= 1e-4 * max(1.0, float(want.abs().max())), f"{what}: {e:.3e}"
            same_bits(runs[1], runs[0], what)
