"""paig_rollout_in_fwd / _bwd (csrc/rollout_in.hip) alone, against the float64
restatement of tests/rollout_in_ref.py.

Tolerance: tests/envelope.py's rule and constants.  The error of pvs, dpos0,
dvel0 and of each of the eight parameter gradients against float64 must be at
most ENVELOPE_K times the largest error of the fp32 CPU ensemble (the
unperturbed weights and ENSEMBLE one-ulp-perturbed copies), with that file's
floor.  Shapes: ragged and exact 16-row tiles, one k-step / several waves / the
largest H, two and six ordered pairs, the spring rollout length at K = 3.
"""
import functools

import numpy as np
import pytest
import torch

import envelope as E
import rollout_in_ref as IR
from helpers import rel_err

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
#        B  D  H    R
CASES = [(1, 4, 4, 1), (5, 4, 12, 3), (17, 6, 20, 4), (16, 6, 128, 5), (37, 4, 100, 12), (33, 6, 100, 46)]
# dense: a dpvs as well; acc: accumulate onto prefilled gradients; vel: a vel0; ld: pos0's row stride - D
VARIANTS = {"plain": dict(dense=0, acc=0, vel=1, ld=0), "dense_acc": dict(dense=1, acc=1, vel=1, ld=0),
            "null_vel": dict(dense=0, acc=0, vel=0, ld=0), "strided": dict(dense=1, acc=0, vel=1, ld=3)}
SATURATED = (37, 4, 100, 12)
OUT = ("pvs", "dpos0", "dvel0") + IR.KEYS
ADJ = (0, 2, 4, 6)   # the weights the adjoint reads: W_r1, W_r2, W_o1, W_o2


def _half(D):
    return 16.0 if D == 4 else 18.0


@functools.lru_cache(maxsize=None)
def _inputs(case, scale=1.0):
    """Seeded fp32 inputs of a case (CPU): weights, pos0, vel0, the adjoints
    and the gradients an accumulating backward starts from."""
    B, D, H, R = case
    g = torch.Generator().manual_seed(1000 * B + R)
    W = {k: v * scale for k, v in IR.default_weights(D, H, seed=7 * B + H).items()}
    rnd = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    d = {"W": W, "pos0": 4 + 24 * rnd(B, D), "vel0": -3 + 6 * rnd(B, D), "dpr": rnd(B, R, D) - 0.5,
         "dpvs": rnd(B, R + 1, 2 * D) - 0.5, "g0": {k: 0.1 * (rnd(*v.shape) - 0.5) for k, v in W.items()}}
    return d


def _cpu(case, var, W, dtype, perm=None):
    """The restatement's outputs and gradients in ``dtype``: {key: float64 numpy}."""
    B, D, H, R = case
    v, inp = VARIANTS[var], _inputs(case)
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)   # noqa: E731  (never the cached input itself)
    W = {k: leaf(t) for k, t in W.items()}
    pos0 = leaf(inp["pos0"] if perm is None else inp["pos0"][:, perm])
    vel0 = leaf((inp["vel0"] if perm is None else inp["vel0"][:, perm]) if v["vel"] else torch.zeros(B, D))
    pvs = IR.rollout(W, pos0, vel0, R, _half(D))
    loss = (pvs[:, 1:, :D] * inp["dpr"].to(dtype)).sum()
    if v["dense"]:
        loss = loss + (pvs * inp["dpvs"].to(dtype)).sum()
    loss.backward()
    out = {"pvs": pvs, "dpos0": pos0.grad, "dvel0": vel0.grad}
    for k in IR.KEYS:
        out[k] = W[k].grad + (inp["g0"][k].to(dtype) if v["acc"] else 0)
    return {k: t.detach().double().numpy() for k, t in out.items()}


@functools.lru_cache(maxsize=None)
def _reference(case, var, scale=1.0, perm=None):
    """(float64 result, [fp32 result, fp32 results on one-ulp-perturbed weights]), computed once."""
    torch.set_num_threads(8)
    W = _inputs(case, scale)["W"]
    perm = None if perm is None else list(perm)
    f64 = _cpu(case, var, W, torch.float64, perm)
    f32 = [_cpu(case, var, W, torch.float32, perm)]
    f32 += [_cpu(case, var, E._ulp_perturbed(W, s), torch.float32, perm) for s in range(E.ENSEMBLE)]
    return f64, f32


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _hip(case, var, scale=1.0, save=True, backward=True, perm=None):
    """One forward (+ backward) on the device.  Every output and the workspace
    are NaN before the launch and carry NaN sentinels past their last row,
    which must survive.  {key: device tensor}."""
    from paig_reproduction_amd._lib import lib, ptr, stream_handle
    L = lib()
    B, D, H, R = case
    v, inp = VARIANTS[var], _inputs(case, scale)
    W = [inp["W"][k].to(DEV).contiguous() for k in IR.KEYS]
    ld = D + v["ld"]
    p0, v0 = (inp["pos0"], inp["vel0"]) if perm is None else (inp["pos0"][:, list(perm)], inp["vel0"][:, list(perm)])
    pos0 = _nan(B, ld)
    pos0[:, :D] = p0.to(DEV)
    vel0 = v0.to(DEV).view(B, D // 2, 2).permute(1, 0, 2).contiguous() if v["vel"] else None
    half = _half(D)
    st = stream_handle(DEV)
    pvs = _nan(B + 1, R + 1, 2 * D)
    nws = L.paig_rollout_in_workspace(B, D, H, R)
    assert nws > 0 and nws % 16 == 0
    ws = _nan(nws // 4 + 4) if (save or backward) else None
    L.paig_rollout_in_fwd(ptr(pos0), ld, ptr(vel0), *[ptr(w) for w in W], half, ptr(pvs), ptr(ws), nws if ws is not None
                          else 0, B, D, H, R, st)
    out = {"pvs": pvs[:B]}
    sent = [pvs[B]] + ([ws[nws // 4:]] if ws is not None else [])
    if backward:
        dpr = inp["dpr"].to(DEV).contiguous()
        dpvs = inp["dpvs"].to(DEV).contiguous() if v["dense"] else None
        dpos0, dvel0 = _nan(B + 1, D), _nan(B * D + 8)
        g = [_nan(w.numel() + 8) for w in W]
        if v["acc"]:
            for t, k in zip(g, IR.KEYS):
                t[:-8] = inp["g0"][k].to(DEV).reshape(-1)
        L.paig_rollout_in_bwd(ptr(dpr), ptr(dpvs), *[ptr(W[i]) for i in ADJ], half, ptr(dpos0),
                              ptr(dvel0) if v["vel"] else None, *[ptr(t) for t in g], v["acc"], ptr(ws), nws, B, D, H,
                              R, st)
        out["dpos0"] = dpos0[:B]
        if v["vel"]:
            out["dvel0"] = dvel0[:B * D].view(D // 2, B, 2).permute(1, 0, 2).reshape(B, D)
        for t, w, k in zip(g, W, IR.KEYS):
            out[k] = t[:-8].view(w.shape)
        sent += [dpos0[B], dvel0[B * D:] if v["vel"] else dvel0] + [t[-8:] for t in g]
    torch.cuda.synchronize()
    for s in sent:
        assert bool(torch.isnan(s).all()), "a sentinel past the last row was written"
    return out


def _check_envelope(case, var, scale=1.0):
    f64, f32 = _reference(case, var, scale)
    hip = _hip(case, var, scale)
    over = {}
    for k in OUT:
        if k == "dvel0" and not VARIANTS[var]["vel"]:
            continue
        got = hip[k].double().cpu().numpy()
        assert np.isfinite(got).all(), f"{k}: non-finite"
        e = rel_err(got, f64[k])
        e32 = max(rel_err(r[k], f64[k]) for r in f32)
        bar = max(E.ENVELOPE_K * e32, E.ENVELOPE_FLOOR)
        print(f"ENVELOPE {case} {var} x{scale:g} {k:16s} hip {e:.2e}  e32 {e32:.2e}  bar {bar:.2e}")
        if not e <= bar:
            over[k] = f"hip {e:.2e} > bar {bar:.2e} (fp32 {e32:.2e})"
    assert not over, over
    return f64


@pytest.mark.parametrize("var", list(VARIANTS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_within_fp32_envelope(case, var):
    f64 = _check_envelope(case, var)
    if not VARIANTS[var]["acc"]:   # not vacuous: every reference gradient is non-zero
        for k in ("dpos0", "dvel0") + IR.KEYS:
            assert float(np.abs(f64[k]).max()) > 0, k
    assert float(np.abs(f64["pvs"][:, 1:, :case[1]] - f64["pvs"][:, :1, :case[1]]).max()) > 1e-3


def test_saturated_tanh_stays_finite_and_within_envelope():
    """All weights x 20: pre-activations far past where (e^2x - 1) / (e^2x + 1) overflows."""
    for var in ("plain", "strided"):
        _check_envelope(SATURATED, var, scale=20.0)


@pytest.mark.parametrize("case", [(17, 6, 20, 4), (33, 6, 100, 46)], ids=lambda c: "x".join(map(str, c)))
def test_repeat_launch_and_null_workspace_are_bit_identical(case):
    a, b = _hip(case, "strided"), _hip(case, "strided")
    assert set(a) == set(b) == set(OUT)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for save in (True, False):
        c = _hip(case, "strided", save=save, backward=False)
        assert torch.equal(c["pvs"], a["pvs"]), f"forward with save={save}"


@pytest.mark.parametrize("case", [(17, 6, 20, 4), (33, 6, 100, 46)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("perm", [(1, 0, 2), (2, 0, 1)])
def test_object_permutation_equivariance_on_the_device(case, perm):
    """The forward of an object-permuted input against the permuted output of
    the unpermuted input, under the envelope bar of the permuted problem (not
    bit for bit: the sum over senders takes another order)."""
    D = case[1]
    cols = tuple(2 * i + c for i in perm for c in (0, 1))
    full = list(cols) + [D + c for c in cols]
    f64, f32 = _reference(case, "plain", 1.0, cols)
    raw = _hip(case, "plain", backward=False)["pvs"].double().cpu().numpy()
    base = raw[:, :, full]
    got = _hip(case, "plain", backward=False, perm=cols)["pvs"].double().cpu().numpy()
    e32 = max(rel_err(r["pvs"], f64["pvs"]) for r in f32)
    bar = max(E.ENVELOPE_K * e32, E.ENVELOPE_FLOOR)
    e_ref, e_perm = rel_err(got, f64["pvs"]), rel_err(got, base)
    print(f"EQUIVARIANCE {case} {perm} vs f64 {e_ref:.2e}  vs permuted output {e_perm:.2e}  bar {bar:.2e}")
    assert e_ref <= bar and e_perm <= bar
    assert float(np.abs(base - raw).max()) > 1e-3   # the permutation moves something


@pytest.mark.parametrize("D,H", [(4, 6), (4, 132), (4, 0), (5, 8), (4, 2)])
def test_unsupported_shape_is_an_error_status(D, H):
    from paig_reproduction_amd._lib import PaigError, lib, ptr, stream_handle
    t = torch.zeros(64, device=DEV)
    with pytest.raises(PaigError, match="1002"):
        lib().paig_rollout_in_fwd(ptr(t), D, None, *[ptr(t)] * 8, 16.0, ptr(t), None, 0, 1, D, H, 1, stream_handle(DEV))
    with pytest.raises(PaigError, match="1002"):
        lib().paig_rollout_in_bwd(ptr(t), None, *[ptr(t)] * 4, 16.0, *[ptr(t)] * 10, 0, ptr(t), 256, 1, D, H, 1,
                                  stream_handle(DEV))


def test_short_workspace_is_an_error_status():
    from paig_reproduction_amd._lib import PaigError, lib, ptr, stream_handle
    t = torch.zeros(256, device=DEV)
    need = lib().paig_rollout_in_workspace(1, 4, 8, 1)
    assert need > 16
    with pytest.raises(PaigError, match="1002"):
        lib().paig_rollout_in_fwd(ptr(t), 4, None, *[ptr(t)] * 8, 16.0, ptr(t), ptr(t), need - 16, 1, 4, 8, 1,
                                  stream_handle(DEV))
    with pytest.raises(PaigError, match="1002"):
        lib().paig_rollout_in_bwd(ptr(t), None, *[ptr(t)] * 4, 16.0, *[ptr(t)] * 10, 0, ptr(t), need - 16, 1, 4, 8, 1,
                                  stream_handle(DEV))
