"""The rollout kernels (paig_rollout_fwd / paig_rollout_bwd, csrc/rollout.hip
and csrc/rollout_cells.h) at states where their physics acts: bouncing
sequences that hit the walls, gravity pairs in each of the force's five clamp
regimes, batches that span several blocks of the serial adjoint, and every
argument form the engine and the module path use.

Reference: autograd through the oracle's cells (oracle/physics_oracle.py)
applied R times in float64 on the CPU, with the spring test's loss (random
adjoints of every step's positions and of the whole pos_vel_seq).  Compared:
the whole pos_vel_seq, d pos0, d vel0 and the physics-parameter gradients.

Bar (tests/envelope.py's rule): ENVELOPE_K times the furthest member of an
fp32 ensemble of the same oracle code (plain fp32, and pos0 / vel0 perturbed
by at most one ulp) from the float64 result, at least ENVELOPE_FLOOR; every
bar must itself be <= 1e-4 (a condition on the inputs).  Errors are normwise
per regime group.  The inputs are chosen by the float64 replay alone
(tests/rollout_cases.py): every branch decision sits a margin away from its
threshold, and every case asserts the coverage it exists for.  Every output
buffer is pre-filled with NaN.
"""
import functools

import numpy as np
import pytest
import torch

import rollout_cases as C
from helpers import rel_err
from rollout_cases import BOUNCE, GRAVITY, SPRING

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 123.25
PAIG_E_SHAPE, PAIG_E_UNSUPPORTED = 1001, 1002
GRAD_KEYS = {SPRING: ("dpos0", "dvel0", "g0", "g1"), BOUNCE: ("dpos0", "dvel0"), GRAVITY: ("dpos0", "dvel0", "g0")}


def L():
    from paig_reproduction_amd._lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def p_(t):
    return None if t is None else t.data_ptr()


def _device_params(cell, prm):
    dt = C.cell_dt(cell).to(DEV)
    names = {SPRING: ("k", "equil"), GRAVITY: ("g", "m"), BOUNCE: ()}[cell]
    return dt, [prm[k].to(DEV) for k in names] or [None, None]


def hip_forward(cell, pos0, vel0, R, prm=None, ld_mult=1):
    """paig_rollout_fwd into a NaN-filled pvs [B, R+1, 2D] (device); vel0 None:
    a null pointer; ld_mult > 1: pos0 rows ld_mult * D apart, NaN between."""
    B, D = pos0.shape
    prm = C.default_params(cell) if prm is None else prm
    dt, (p0, p1) = _device_params(cell, prm)
    pbuf = torch.full((B, ld_mult * D), NAN)
    pbuf[:, :D] = pos0
    pg = pbuf.to(DEV)
    vk = None if vel0 is None else vel0.view(B, D // 2, 2).permute(1, 0, 2).contiguous().to(DEV)
    pvs = torch.full((B, R + 1, 2 * D), NAN, device=DEV)
    assert L().paig_rollout_fwd(cell, p_(pg), ld_mult * D, p_(vk), p_(dt), p_(p0), p_(p1), p_(pvs), B, D, R, st()) == 0
    torch.cuda.synchronize()
    return pvs


def hip_rollout(cell, pos0, vel0, R, dpos_roll, dpvs, prm=None, ld_mult=1, null_dvel0=False, prefill=None):
    """Forward and adjoint on the device.  prefill: (a, b) -> accumulate = 1
    onto those gparam values.  Returns {pvs, dpos0, dvel0 [B, D], g0, g1}
    (float64 numpy; g* as left in the gparam buffer)."""
    B, D = pos0.shape
    prm = C.default_params(cell) if prm is None else prm
    dt, (p0, p1) = _device_params(cell, prm)
    pvs = hip_forward(cell, pos0, vel0, R, prm, ld_mult)
    assert bool(torch.isfinite(pvs).all()), "pos_vel_seq not fully written"
    dpos0 = torch.full((B, D), NAN, device=DEV)
    dvel0 = None if null_dvel0 else torch.full((D // 2, B, 2), NAN, device=DEV)
    nrow = L().paig_rollout_bwd_blocks(B)
    assert nrow >= -(-B // 64)
    part = torch.full((2 * nrow,), NAN, device=DEV, dtype=torch.float64)
    # gparam: NaN where the kernel must write, a sentinel where it must not
    # (bouncing has no parameters; gravity's mass has no gradient)
    fill = {SPRING: (NAN, NAN), BOUNCE: (SENTINEL, SENTINEL), GRAVITY: (NAN, SENTINEL)}[cell] if prefill is None else prefill
    gq = torch.tensor(fill, dtype=torch.float64, device=DEV)
    dr = None if dpos_roll is None else dpos_roll.to(DEV).contiguous()
    dv = None if dpvs is None else dpvs.to(DEV).contiguous()
    assert L().paig_rollout_bwd(cell, p_(pvs), p_(dr), p_(dv), p_(dt), p_(p0), p_(p1), p_(dpos0), p_(dvel0), p_(part),
                                p_(gq), p_(gq) + 8, 0 if prefill is None else 1, B, D, R, st()) == 0
    torch.cuda.synchronize()
    out = {"pvs": pvs, "dpos0": dpos0, "g0": gq[0:1], "g1": gq[1:2]}
    if dvel0 is not None:
        out["dvel0"] = dvel0.permute(1, 0, 2).reshape(B, D)
    return {k: v.double().cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _case(cell, kind, B, R):
    """(pos0, vel0, replay, dpos_roll, dpvs, float64 reference, fp32 ensemble), computed once."""
    if cell == BOUNCE:
        pos0, vel0, rep = C.bouncing_overshoot_inputs(B, R) if kind == "overshoot" else \
            C.bouncing_inputs(B, R, seed=2 if B == 1 else 0)
    elif cell == GRAVITY:
        pos0, vel0, rep = C.gravity_inputs(kind, B, R)
    else:
        pos0, vel0, dr, dv = C.spring_inputs(B, R)
        return (pos0, vel0, None, dr, dv) + C.reference(cell, pos0, vel0, R, dr, dv)
    dr, dv = C.adjoints(B, R, pos0.shape[1], 31 * B + R)
    return (pos0, vel0, rep, dr, dv) + C.reference(cell, pos0, vel0, R, dr, dv)


def _judge(what, got, f64, f32, keys, rows=None):
    """Print and assert the envelope bars of ``keys`` over the sequences ``rows``."""
    bad = []
    for k, (e, e32, bar) in C.envelope_rows(got, f64, f32, keys, rows).items():
        print(f"ENVELOPE {what:34s} {k:6s} kernel {e:.2e}  e32 {e32:.2e}  bar {bar:.2e}")
        assert bar <= C.NORTH_STAR, f"{what}: the inputs put the {k} bar at {bar:.2e} > 1e-4"
        if not e <= bar:
            bad.append(f"{k}: {e:.3e} > {bar:.3e}")
    assert not bad, f"{what}: {bad}"


# ---------------------------------------------------------------- bouncing ----
def _bouncing_checks(pos0, vel0, R, dr, dv, got, f64):
    """What holds exactly for the bouncing cell: velocities only ever change
    sign (bit-equal to the float64 replay's), and columns 2, 3 never move
    (split-size-1 quirk): their adjoints are the plain sums of the injections."""
    pvs = got["pvs"]
    assert np.array_equal(pvs[:, :, 4:], f64["pvs"][:, :, 4:]), "a velocity is not +-vel0 as in the float64 replay"
    for t in range(R + 1):
        assert np.array_equal(pvs[:, t, 2:4], pos0[:, 2:4].double().numpy())
        assert np.array_equal(pvs[:, t, 6:8], vel0[:, 2:4].double().numpy())
    # a serial fp32 sum of n terms is within n 2^-24 sum|x| of the exact one
    terms_p = torch.cat([dr[:, :, 2:4], dv[:, :, 2:4]], 1).double()
    terms_v = dv[:, :, 6:8].double()
    for key, terms in (("dpos0", terms_p), ("dvel0", terms_v)):
        tol = terms.shape[1] * 2.0 ** -24 * terms.abs().sum(1).numpy()
        assert (np.abs(got[key][:, 2:4] - terms.sum(1).numpy()) <= tol).all(), key


@pytest.mark.parametrize("B,R,min_hits", [(1, 1, 0), (64, 2, 5), (65, 20, 20), (130, 20, 20), (5, 96, 20)])
def test_bouncing_walls(B, R, min_hits):
    """Sequences that hit the walls (pos0 ~ U[4, 28], vel0 ~ U[-40, 40]):
    bounce_sub's flags a, b, c and bounce_sub_bwd's sign flips; 65 and 130
    sequences: two and three partial rows; R = 96: bench's longest rollout."""
    pos0, vel0, rep, dr, dv, f64, f32 = _case(BOUNCE, "walls", B, R)
    hits = torch.stack([rep["up"].sum(0), rep["low"].sum(0)])      # [wall, column]
    print(f"bouncing B={B} R={R}: upper-wall hits {hits[0].tolist()}, lower-wall hits {hits[1].tolist()}, "
          f"margin {float(rep['margin'].min()):.2e}")
    assert int(hits.sum()) >= 1
    assert int(hits.min()) >= min_hits, hits.tolist()
    if R >= 20:
        assert bool(((rep["up"] > 0) & (rep["low"] > 0)).any()), "no sequence hits both walls on one column"
    got = hip_rollout(BOUNCE, pos0, vel0, R, dr, dv)
    _bouncing_checks(pos0, vel0, R, dr, dv, got, f64)
    assert got["g0"][0] == SENTINEL and got["g1"][0] == SENTINEL, "bouncing has no parameters to write"
    _judge(f"bouncing B={B} R={R}", got, f64, f32, ("pvs",) + GRAD_KEYS[BOUNCE])


def test_bouncing_overshoot():
    """|vel0[:, 0]| > 480: a substep overshoots the far wall so far that the
    reflected position lies beyond the near wall (flags a and c together)."""
    pos0, vel0, rep, dr, dv, f64, f32 = _case(BOUNCE, "overshoot", 8, 2)
    assert bool((vel0[:, 0].abs() > 480).all()) and bool((rep["ac"] >= 1).all()), rep["ac"].tolist()
    got = hip_rollout(BOUNCE, pos0, vel0, 2, dr, dv)
    _bouncing_checks(pos0, vel0, 2, dr, dv, got, f64)
    _judge("bouncing overshoot B=8 R=2", got, f64, f32, ("pvs",) + GRAD_KEYS[BOUNCE])


# ----------------------------------------------------------------- gravity ----
def _regime_line(group, rep):
    n = rep["counts"].sum(0).tolist()
    return f"gravity {group}: pair-substeps " + ", ".join(f"{r} {c}" for r, c in zip(C.REGIMES, n))


@pytest.mark.parametrize("B,R", [(1, 1), (64, 2), (65, 6), (130, 12)])
def test_gravity_free(B, R):
    """The unclamped regime 1 <= |r| <= 170 (every pair >= 3 px apart at every
    substep): the force's 1 / |r|^3 and the -3 vec / |r|^5 terms of its adjoint."""
    pos0, vel0, rep, dr, dv, f64, f32 = _case(GRAVITY, "free", B, R)
    print(_regime_line("free", rep), f"closest approach {float(rep['dmin'].min()):.2f} px")
    assert int(rep["counts"][:, 2].sum()) == 15 * R * B and float(rep["dmin"].min()) >= C.GRAV_FREE_MIN
    got = hip_rollout(GRAVITY, pos0, vel0, R, dr, dv)
    assert got["g1"][0] == SENTINEL, "the mass has no gradient: gparam1 must stay untouched"
    _judge(f"gravity free B={B} R={R}", got, f64, f32, ("pvs",) + GRAD_KEYS[GRAVITY])


@pytest.mark.parametrize("group,R", [("near", 1), ("touching", 1), ("touching", 2), ("far", 1), ("far", 2),
                                     ("veryfar", 1), ("veryfar", 2)])
def test_gravity_clamp_regimes(group, R):
    """One pair inside a clamp: near (sq >= 0.1, nrm < 1), touching (sq < 0.1),
    far (nrm > 170, sq <= 1e5), very far (sq > 1e5).  The g gradient is judged
    in the far groups only: in the near ones the fp32 reference itself loses
    it to cancellation."""
    B = 16
    pos0, vel0, rep, dr, dv, f64, f32 = _case(GRAVITY, group, B, R)
    own = C.REGIMES.index(group)
    print(_regime_line(group, rep), f"margin {float(rep['margin'].min()):.3f}")
    assert bool((rep["counts"][:, own] > 0).all()) and float(rep["margin"].min()) >= C.GRAV_MARGIN
    got = hip_rollout(GRAVITY, pos0, vel0, R, dr, dv)
    assert got["g1"][0] == SENTINEL
    assert np.isfinite(got["g0"][0])
    keys = ("pvs", "dpos0", "dvel0") + (("g0",) if group in ("far", "veryfar") else ())
    _judge(f"gravity {group} B={B} R={R}", got, f64, f32, keys)


@functools.lru_cache(maxsize=None)
def _gravity_mixed(R=2):
    groups = [("free", 65)] + [(g, 16) for g in ("near", "touching", "far", "veryfar")]
    parts = [C.gravity_inputs(g, B, R) for g, B in groups]
    pos0, vel0 = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    rows, at = {}, 0
    for (g, B), p in zip(groups, parts):
        rows[g] = slice(at, at + B)
        at += B
        assert int(p[2]["counts"][:, C.REGIMES.index(g)].sum()) > 0
    dr, dv = C.adjoints(at, R, 6, 5)
    return (pos0, vel0, rows, dr, dv) + C.reference(GRAVITY, pos0, vel0, R, dr, dv)


def test_gravity_regimes_in_one_batch():
    """The five groups in one batch of 129 (three partial rows), each judged
    on its own rows: a clamp-regime gradient is small beside the free ones."""
    pos0, vel0, rows, dr, dv, f64, f32 = _gravity_mixed()
    got = hip_rollout(GRAVITY, pos0, vel0, 2, dr, dv)
    assert got["g1"][0] == SENTINEL
    for g, sl in rows.items():
        _judge(f"gravity mixed R=2 [{g}]", got, f64, f32, ("pvs", "dpos0", "dvel0"), sl)
    _judge("gravity mixed R=2 [batch]", got, f64, f32, ("g0",))


# ------------------------------------------------------------------ spring ----
@pytest.mark.parametrize("B,R", [(37, 6), (130, 65)])
def test_spring_forward_and_serial_rows(B, R):
    """The spring forward's whole pos_vel_seq under the envelope rule, and
    (130, 65) the serial adjoint (R > 64) over three partial rows, at the
    spring test's recipe and its 1e-4 bar."""
    pos0, vel0, _, dr, dv, f64, f32 = _case(SPRING, "spring", B, R)
    n = np.abs(f64["pvs"][:, :, 0] - f64["pvs"][:, :, 1]).min()
    assert n >= 1.0, f"the spring passes n = {n:.2f}: d / (n + 1e-4) decorrelates any fp32 run"
    got = hip_rollout(SPRING, pos0, vel0, R, dr, dv)
    for t in range(R + 1):   # columns 2, 3 never move
        assert np.array_equal(got["pvs"][:, t, 2:4], pos0[:, 2:4].double().numpy())
    _judge(f"spring B={B} R={R}", got, f64, f32, ("pvs",))
    for k in GRAD_KEYS[SPRING]:
        e = rel_err(got[k], f64[k])
        print(f"SPRING B={B} R={R} {k} kernel {e:.2e}  bar 1.00e-04")
        assert e <= 1e-4, (k, e)


# ---------------------------------------------------------- argument forms ----
FORM_R = {SPRING: 3, BOUNCE: 4, GRAVITY: 2}
SPRING_FORM_SEED = 8   # (of seeds 1-8 one whose k gradient does not cancel in fp32: bars <= 3e-5 for every form)
FORMS = ("null_vel0", "pos0_ld", "null_dpos_roll", "null_dpvs", "null_dvel0", "accumulate")


@functools.lru_cache(maxsize=None)
def _form_reference(cell, form):
    B, R = 65, FORM_R[cell]
    if cell == BOUNCE:
        pos0, vel0, _ = C.bouncing_inputs(B, R, seed=9)
    elif cell == GRAVITY:
        pos0, vel0, _ = C.gravity_inputs("free", B, R, seed=9)
    # (gravity: of seeds 40-46 one whose g gradient does not cancel in fp32 in any form: e32 <= 5e-6)
    dr, dv = C.adjoints(B, R, C.CELL_D[cell], 40 if cell == GRAVITY else 18)
    if cell == SPRING:
        pos0, vel0, dr, dv = C.spring_inputs(B, R, seed=SPRING_FORM_SEED)
    if form == "null_vel0":
        vel0 = torch.zeros_like(vel0)
    if form == "null_dpos_roll":
        dr = None
    if form == "null_dpvs":
        dv = None
    if cell != SPRING:   # the margins of the inputs as this form runs them
        C.assert_margins(cell, pos0, vel0, R, "free")
    return (pos0, vel0, dr, dv) + C.reference(cell, pos0, vel0, R, dr, dv)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cell", [SPRING, BOUNCE, GRAVITY])
def test_argument_forms(cell, form):
    """Every argument form the engine and the module path take, at B = 65
    (two partial rows of the serial adjoint, 17 of the spring scan), against
    the float64 reference with the corresponding term dropped; `part` is
    sized exactly and NaN-filled."""
    pos0, vel0, dr, dv, f64, f32 = _form_reference(cell, form)
    R = FORM_R[cell]
    kw = {}
    if form == "pos0_ld":
        kw["ld_mult"] = 3
    if form == "null_dvel0":
        kw["null_dvel0"] = True
    if form == "accumulate":
        kw["prefill"] = (1.5, -2.25)
    got = hip_rollout(cell, pos0, None if form == "null_vel0" else vel0, R, dr, dv, **kw)
    keys = ("pvs",) + GRAD_KEYS[cell]
    if form == "null_dvel0":
        keys = tuple(k for k in keys if k != "dvel0")
    if form == "accumulate":   # the result is the pre-fill plus the gradient; untouched where there is none
        written = {SPRING: 2, BOUNCE: 0, GRAVITY: 1}[cell]
        for i, fill in enumerate(kw["prefill"]):
            if i < written:
                got[f"g{i}"] = got[f"g{i}"] - fill
            else:
                assert got[f"g{i}"][0] == fill, f"gparam{i} touched"
    elif cell == GRAVITY:
        assert got["g1"][0] == SENTINEL
    _judge(f"{('spring', 'bouncing', 'gravity')[cell]} {form}", got, f64, f32, keys)


def test_unsupported_and_missing_parameters():
    """Argument checks that return before any launch: a cell / D pair with no
    kernel is PAIG_E_UNSUPPORTED with a message; spring and gravity without
    their parameters are rejected; nothing is written."""
    lib = L()
    fwd, bwd = lib.fns["paig_rollout_fwd"], lib.fns["paig_rollout_bwd"]
    B, R = 3, 2
    dt = C.cell_dt(GRAVITY).to(DEV)
    q = torch.zeros(2, dtype=torch.float64, device=DEV)
    for cell, D in ((GRAVITY, 4), (BOUNCE, 6)):
        pos0, vel0 = torch.full((B, D), 16.0, device=DEV), torch.zeros(D // 2, B, 2, device=DEV)
        pvs = torch.full((B, R + 1, 2 * D), NAN, device=DEV)
        rc = fwd(cell, p_(pos0), D, p_(vel0), p_(dt), p_(q), p_(q) + 8, p_(pvs), B, D, R, st())
        assert rc == PAIG_E_UNSUPPORTED, rc
        msg = lib.paig_last_error().decode()
        assert "unsupported" in msg and f"D={D}" in msg, msg
        dpos0 = torch.full((B, D), NAN, device=DEV)
        part = torch.full((2 * lib.paig_rollout_bwd_blocks(B),), NAN, device=DEV, dtype=torch.float64)
        rc = bwd(cell, p_(pvs), None, None, p_(dt), p_(q), p_(q) + 8, p_(dpos0), None, p_(part), p_(q), p_(q) + 8, 0,
                 B, D, R, st())
        assert rc == PAIG_E_UNSUPPORTED, rc
        torch.cuda.synchronize()
        assert bool(torch.isnan(pvs).all()) and bool(torch.isnan(dpos0).all()) and bool(torch.isnan(part).all())
    for cell, D in ((SPRING, 4), (GRAVITY, 6)):
        pos0 = torch.full((B, D), 16.0, device=DEV)
        pvs = torch.full((B, R + 1, 2 * D), NAN, device=DEV)
        rc = fwd(cell, p_(pos0), D, None, p_(dt), None, p_(q) + 8, p_(pvs), B, D, R, st())
        assert rc == PAIG_E_SHAPE, rc
        assert "physics params required" in lib.paig_last_error().decode()
        dpos0 = torch.full((B, D), NAN, device=DEV)
        part = torch.full((2 * lib.paig_rollout_bwd_blocks(B),), NAN, device=DEV, dtype=torch.float64)
        rc = bwd(cell, p_(pvs), None, None, p_(dt), None, p_(q) + 8, p_(dpos0), None, p_(part), p_(q), p_(q) + 8, 0,
                 B, D, R, st())
        assert rc == PAIG_E_SHAPE, rc
        torch.cuda.synchronize()
        assert bool(torch.isnan(pvs).all()) and bool(torch.isnan(dpos0).all())
    assert bool((q == 0).all())


# ----------------------------------------------------------- merged launch ----
@pytest.mark.parametrize("cell,K,H,kind,B,R", [(BOUNCE, 2, 32, "walls", 65, 20), (GRAVITY, 3, 36, "free", 65, 6)])
def test_merged_launch_rollout_bit_identical(cell, K, H, kind, B, R):
    """paig_decoder_fwd_rollout runs the same rollout_fwd_seq inside
    decoder.hip: its pos_vel_seq is paig_rollout_fwd's bit for bit at states
    that bounce / attract, and its decode is paig_decoder_fwd's."""
    from test_gpu_decoder import _fwd, _positions, _sources
    pos0, vel0 = _case(cell, kind, B, R)[:2]
    D, F_, fr = 2 * K, 7, 3 * H * H
    want = hip_forward(cell, pos0, vel0, R)
    tmpl, cont, bg = _sources(K, H, 21 + K)
    pos = _positions(F_, K, H, 4).to(DEV).contiguous()
    tgt = torch.rand(F_, 3, H, H, generator=torch.Generator().manual_seed(6)).to(DEV).contiguous()
    td, cd, bd = tmpl.to(DEV).contiguous(), cont.to(DEV).contiguous(), bg.to(DEV).contiguous()
    dt, (p0, p1) = _device_params(cell, C.default_params(cell))
    pg = pos0.to(DEV)
    vk = vel0.view(B, K, 2).permute(1, 0, 2).contiguous().to(DEV)
    pvs = torch.full((B, R + 1, 2 * D), NAN, device=DEV)
    out = torch.full((F_, 3, H, H), NAN, device=DEV)
    sse = torch.full((F_,), NAN, device=DEV)
    assert L().paig_decoder_fwd_rollout(cell, p_(pg), D, p_(vk), p_(dt), p_(p0), p_(p1), p_(pvs), B, D, R, p_(pos), 0,
                                        2 * K, 0, p_(td), p_(cd), p_(bd), p_(out), fr, p_(tgt), fr, 0, 0, p_(sse), F_,
                                        K, H // 2, H, st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(pvs, want)
    out1, sse1 = _fwd(K, H, tmpl, cont, bg, (pos.data_ptr(), 0, 2 * K, 0), (tgt.data_ptr(), fr, 0, 0), F_)
    assert torch.equal(out.cpu(), out1) and torch.equal(sse.cpu(), sse1)
