"""CPU checks of tests/unet_glue_ref.py, the reference the GPU tests of the
U-Net pool and upsample kernels compare with (tests/test_gpu_unet_glue.py):
on every shape those tests use, the pool against F.max_pool2d (values, argmax,
NaN rule) and its autograd, the upsample against F.interpolate(mode="bilinear",
align_corners=False, antialias=True) -- nn/network/blocks.py's Resize -- and its
autograd in float64.  Then the inputs, drawn as the GPU tests draw them
(R.rng): that they hold the ties, the ReLU' zeros and the NaNs without which a
wrong kernel would pass.  Last, that the host conditions the GPU test's
docstring quotes are still in the kernels' source.  No GPU."""
import os
import re

import pytest
import torch
import torch.nn.functional as Fn

import unet_glue_ref as R
from helpers import rel_err

TOL = 1e-12
_id = lambda c: "x".join(map(str, c))   # noqa: E731


def _aten_pool(x):
    """F.max_pool2d's values and its argmax as a window position 0..3"""
    y, idx = Fn.max_pool2d(x, 2, return_indices=True)
    W = x.shape[-1]
    return y, (((idx // W) & 1) << 1) | ((idx % W) & 1)


# --------------------------------------------------------------------- pool --
@pytest.mark.parametrize("fc", R.POOL_FC, ids=_id)
@pytest.mark.parametrize("hw", R.POOL_HW, ids=_id)
def test_pool_reference_is_aten_max_pool2d(hw, fc):
    for make in (R.ties, R.gauss):
        g = R.rng(*hw, fc)
        x = make(g, *fc, *hw)
        y, am = R.pool_fwd(x)
        ya, ama = _aten_pool(x)
        assert y.dtype == torch.float32 and torch.equal(y, ya), make.__name__
        assert torch.equal(am, ama), f"{make.__name__}: argmax (the tie rule)"
        # backward: aten scatters dy to its argmax; then the one add and the ReLU' mask
        xr = x.clone().requires_grad_(True)
        dy, dx0 = torch.randn(y.shape, generator=g), torch.randn(x.shape, generator=g)
        Fn.max_pool2d(xr, 2).backward(dy)
        want = torch.where(x > 0, dx0 + xr.grad, torch.zeros_like(x))
        got = R.pool_bwd_relu(x, dy, dx0)
        assert got.dtype == torch.float32 and torch.equal(got, want), make.__name__
        # a trailing odd row / column takes no gradient: dx0 under the mask
        H2, W2 = hw[0] // 2 * 2, hw[1] // 2 * 2
        edge = torch.ones(x.shape, dtype=torch.bool)
        edge[..., :H2, :W2] = False
        assert torch.equal(got[edge], torch.where(x > 0, dx0, torch.zeros_like(x))[edge])


@pytest.mark.parametrize("fc", R.POOL_FC, ids=_id)
@pytest.mark.parametrize("hw", R.POOL_HW, ids=_id)
def test_pool_reference_nan_rule_is_atens(hw, fc):
    x = R.with_nans(R.rng(*hw, fc), *fc, *hw)
    for k, t in enumerate(R._taps(x)):
        assert bool(torch.isnan(t).any()), f"no NaN at window position {k}"
    y, am = R.pool_fwd(x)
    ya, ama = _aten_pool(x)
    assert bool(torch.isnan(y).any()) and (y.numel() <= 4 or not bool(torch.isnan(y).all()))
    assert torch.equal(torch.isnan(y), torch.isnan(ya))
    assert torch.equal(torch.nan_to_num(y), torch.nan_to_num(ya))
    assert torch.equal(am, ama), "argmax with NaNs: the last NaN of a window is taken"


@pytest.mark.parametrize("fc", R.POOL_FC, ids=_id)
@pytest.mark.parametrize("hw", R.CODE_HW, ids=_id)
def test_pool_codes_layout(hw, fc):
    """every byte spelt out from the definition, element by element"""
    F, C = fc
    H, W = hw
    assert hw in R.POOL_HW
    x = R.ties(R.rng(*hw, fc), F, C, H, W)
    code = R.pool_codes(x)
    assert code.dtype == torch.uint8 and code.shape == (F, (C + 7) // 8, H // 2, W // 2, 8)
    _, am = R.pool_fwd(x)
    for f in range(F):
        for c in range(C):
            for i in range(H // 2):
                for j in range(W // 2):
                    px = [x[f, c, 2 * i, 2 * j], x[f, c, 2 * i, 2 * j + 1], x[f, c, 2 * i + 1, 2 * j],
                          x[f, c, 2 * i + 1, 2 * j + 1]]
                    want = sum(int(v > 0) << k for k, v in enumerate(px)) | (int(am[f, c, i, j]) << 4)
                    assert int(code[f, c // 8, i, j, c % 8]) == want
    assert torch.equal(R.codes_by_channel(code, C)[:, C - 1], code[:, (C - 1) // 8, :, :, (C - 1) % 8])


# ----------------------------------------------------------------- upsample --
def test_up_matrix_rows():
    assert torch.equal(R.up_matrix(1), torch.ones(2, 1, dtype=torch.float64))
    M = R.up_matrix(3)
    want = torch.tensor([[1, 0, 0], [.75, .25, 0], [.25, .75, 0], [0, .75, .25], [0, .25, .75], [0, 0, 1]],
                        dtype=torch.float64)
    assert torch.equal(M, want)
    for n in (1, 2, 5, 9, 128):
        M = R.up_matrix(n)
        assert torch.equal(M.sum(1), torch.ones(2 * n, dtype=torch.float64))       # an interpolation
        assert torch.equal(M.sum(0), torch.full((n,), 2.0, dtype=torch.float64))   # exact 2x: the adjoint's weights


# with the shapes of the upsample's second-trip cases (F aside) and the partial-wave case's (F, C)
@pytest.mark.parametrize("fc", R.UP_FC + [R.PARTIAL_WAVE[2], (2, 2)], ids=_id)
@pytest.mark.parametrize("hw", R.UP_HW + [(1, 4), (4, 256), (8, 8)], ids=_id)
def test_upsample_reference_is_aten_bilinear(hw, fc):
    g = R.rng(*hw, fc)
    Hs, Ws = hw
    s32 = R.gauss(g, *fc, Hs, Ws)
    sr = s32.double().requires_grad_(True)
    u = Fn.interpolate(sr, size=(2 * Hs, 2 * Ws), mode="bilinear", align_corners=False, antialias=True)
    du32 = torch.randn(u.shape, generator=g)
    u.backward(du32.double())
    got, a = R.up_fwd(s32)
    assert got.dtype == torch.float64 and rel_err(got, u.detach()) <= TOL
    assert rel_err(a, Fn.interpolate(s32.double().abs(), size=(2 * Hs, 2 * Ws), mode="bilinear",
                                     align_corners=False, antialias=True)) <= TOL
    ds, a = R.up_bwd(du32)
    assert float(sr.grad.abs().max()) > 0 and rel_err(ds, sr.grad) <= TOL
    assert bool((a >= ds.abs() * (1 - 1e-15)).all())
    dsm, am = R.up_bwd(du32, s32)
    assert rel_err(dsm, sr.grad * (s32 > 0)) <= TOL
    assert bool((dsm[s32 <= 0] == 0).all()) and bool((am[s32 <= 0] == 0).all())
    assert torch.equal(am[s32 > 0], a[s32 > 0])


# --------------------------------------------------------------- generators --
# A shape needs some size before a property of random data can be asked of it:
# a 2 x 2 frame of 3 channels has 3 windows, a 1 x 1 source of one channel has
# one element.  The thresholds are where the property is certain enough to pin
# with a fixed seed; the smaller shapes are run for their addressing.
def _tie_facts(x):
    """(windows with a tied maximum, the argmax, per position: it holds a tied maximum)"""
    m, am = R.pool_fwd(x)
    at = [t == m for t in R._taps(x)]
    tied = sum(a.to(torch.int64) for a in at) >= 2
    return tied, am, [a & tied for a in at]


# With the strict ">" a tied maximum is never taken at position 3 (an earlier
# pixel holds the same value and keeps it), so "argmax 3 with a tie" cannot
# occur.  What exposes a ">=" (or a reversed scan) is a tied maximum *standing*
# at every position 0..3 while the argmax is the first of them: argmax 0, 1, 2
# each occur tied, and position 3 holds a tied maximum that must not win.
@pytest.mark.parametrize("fc", R.POOL_FC, ids=_id)
@pytest.mark.parametrize("hw", R.POOL_HW, ids=_id)
def test_tie_generator_holds_ties_at_every_argmax(hw, fc):
    x = R.ties(R.rng(*hw, fc), *fc, *hw)
    assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0, 2.0}
    tied, am, holds = _tie_facts(x)
    if tied.numel() >= 100:
        assert float(tied.float().mean()) >= 0.25
        for k in range(4):
            assert bool((am == k).any()), f"argmax {k} never occurs"
            assert bool(holds[k].any()), f"position {k} never holds a tied maximum"
            if k < 3:
                assert bool(((am == k) & tied).any()), f"argmax {k} never occurs with a tied maximum"
        assert not bool(((am == 3) & tied).any())


def test_tie_generator_over_all_shapes():
    """the small shapes together: a quarter of all windows tied, a tie standing at every position"""
    tied_n, n, seen, held = 0, 0, set(), set()
    for hw in R.POOL_HW:
        for fc in R.POOL_FC:
            tied, am, holds = _tie_facts(R.ties(R.rng(*hw, fc), *fc, *hw))
            tied_n, n = tied_n + int(tied.sum()), n + tied.numel()
            seen |= set(am[tied].tolist())
            held |= {k for k in range(4) if bool(holds[k].any())}
    assert tied_n >= 0.25 * n and seen == {0, 1, 2} and held == {0, 1, 2, 3}


def _mask_conditions(x):
    n = x.numel()
    if n >= 2:
        z = x.view(-1)[x.view(-1) == 0]
        sign = torch.signbit(z)
        assert bool((~sign).any()) and bool(sign.any()), "needs an exact 0.0 and a -0.0"
    if n >= 32:
        assert 0.2 <= float((x <= 0).float().mean()) <= 0.8


@pytest.mark.parametrize("fc", R.POOL_FC, ids=_id)
@pytest.mark.parametrize("hw", R.POOL_HW, ids=_id)
def test_pool_inputs_exercise_the_relu_mask(hw, fc):
    for make in (R.ties, R.gauss):
        _mask_conditions(make(R.rng(*hw, fc), *fc, *hw))


@pytest.mark.parametrize("fc", R.UP_FC + [R.PARTIAL_WAVE[2]], ids=_id)
@pytest.mark.parametrize("hw", R.UP_HW, ids=_id)
def test_upsample_inputs_exercise_the_relu_mask(hw, fc):
    _mask_conditions(R.gauss(R.rng(*hw, fc), *fc, *hw))


@pytest.mark.parametrize("case", R.SECOND, ids=lambda c: c[0])
def test_second_trip_inputs(case):
    """the large-F inputs of the grid-stride cases: the reference against aten
    at that size, and the same conditions on the data"""
    _, kernel, H, W, per_frame, _ = case
    F, C = R.frames_for(per_frame), 2
    g = R.rng(H, W, (F, C))
    if kernel.startswith("pool"):
        x = R.ties(g, F, C, H, W)
        y, am = R.pool_fwd(x)
        ya, ama = _aten_pool(x)
        assert torch.equal(y, ya) and torch.equal(am, ama)
        tied, am, holds = _tie_facts(x)
        assert float(tied.float().mean()) >= 0.25 and all(bool(h.any()) for h in holds)
        assert all(bool(((am == k) & tied).any()) for k in range(3))
        _mask_conditions(x)
        # the last thousand work items, the second trip's, hold ties too
        assert bool(tied.reshape(-1)[-500:].any())
    else:
        s32 = R.gauss(g, F, C, H, W)
        _mask_conditions(s32)
        assert 0.2 <= float((s32.reshape(-1)[-1000:] <= 0).float().mean()) <= 0.8
        u = Fn.interpolate(s32.double(), size=(2 * H, 2 * W), mode="bilinear", align_corners=False, antialias=True)
        assert rel_err(R.up_fwd(s32)[0], u) <= TOL


# ----------------------------------------------------------------- dispatch --
def test_quoted_dispatch_conditions_are_the_sources():
    """every ``quotation`` in the docstring of tests/test_gpu_unet_glue.py is in
    unet_ops.hip or misc.hip, whitespace aside: its case ids name forms chosen
    by exactly these conditions"""
    import test_gpu_unet_glue as T
    here = os.path.dirname(os.path.abspath(__file__))
    squash = lambda s: re.sub(r"\s+", " ", s)   # noqa: E731
    src = "".join(squash(open(os.path.join(here, "..", "paig_reproduction_amd", "csrc", f)).read())
                  for f in ("unet_ops.hip", "misc.hip"))
    quotes = re.findall(r"``(.+?)``", T.__doc__, re.S)
    assert quotes
    for q in quotes:
        assert squash(q) in src, f"no longer in the source: {q}"
