"""The opt-in 2-D rollout cells (paig_rollout_fwd / paig_rollout_bwd kinds 3
and 4, csrc/rollout_cells.h: spring2d_sub / bounce2d_sub and their adjoints on
the generic serial adjoint), in the style of test_gpu_rollout_cells.py.

Reference: autograd through the float64 restatement of the cells with split
size 2 (tests/rollout2d_cases.py, tied to the pinned oracle at split size 1 by
tests/test_rollout2d_ref_cpu.py), with random adjoints of every step's
positions and of the whole pos_vel_seq.  Compared: the whole pos_vel_seq,
d pos0, d vel0 and the physics-parameter gradients.

Bar (tests/envelope.py's rule): ENVELOPE_K times the furthest member of an
fp32 ensemble of the same restatement from the float64 result, at least
ENVELOPE_FLOOR; every bar must itself be <= 1e-4 (a condition on the inputs,
which the float64 replay alone chooses).  Every output buffer is pre-filled
with NaN and `part` is sized exactly.
"""
import functools

import numpy as np
import pytest
import torch

import rollout2d_cases as C2
import rollout_cases as C
from rollout2d_cases import BOUNCE2D, SPRING2D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 123.25
PAIG_E_SHAPE, PAIG_E_UNSUPPORTED = 1001, 1002
D = 4
GRAD_KEYS = {SPRING2D: ("dpos0", "dvel0", "g0", "g1"), BOUNCE2D: ("dpos0", "dvel0")}
NAME = {SPRING2D: "spring 2-D", BOUNCE2D: "bouncing 2-D"}
# (37, 65): of seeds 0-9 the one at which every bar of the fp32 ensemble is <= 1e-4 (R = 65 steps of an
# oscillator with close approaches: the fp32 reference itself sits at 2e-5 .. 3e-4 from float64)
SPRING_SEED = {(37, 65): 2}


def L():
    from paig_reproduction_amd._lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def p_(t):
    return None if t is None else t.data_ptr()


def _device_params(cell, prm):
    dt = C2.cell_dt().to(DEV)
    return dt, [prm[k].to(DEV) for k in C2.PARAM_NAMES[cell]] or [None, None]


def hip_forward(cell, pos0, vel0, R, prm=None, ld_mult=1):
    """paig_rollout_fwd into a NaN-filled pvs [B, R+1, 2D] (device); vel0 None:
    a null pointer; ld_mult > 1: pos0 rows ld_mult * D apart, NaN between."""
    B = pos0.shape[0]
    prm = C2.default_params(cell) if prm is None else prm
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
    B = pos0.shape[0]
    prm = C2.default_params(cell) if prm is None else prm
    dt, (p0, p1) = _device_params(cell, prm)
    pvs = hip_forward(cell, pos0, vel0, R, prm, ld_mult)
    assert bool(torch.isfinite(pvs).all()), "pos_vel_seq not fully written"
    dpos0 = torch.full((B, D), NAN, device=DEV)
    dvel0 = None if null_dvel0 else torch.full((D // 2, B, 2), NAN, device=DEV)
    nrow = L().paig_rollout_bwd_blocks(B)
    assert nrow >= -(-B // 64)
    part = torch.full((2 * nrow,), NAN, device=DEV, dtype=torch.float64)
    # gparam: NaN where the kernel must write, a sentinel where it must not (bouncing has no parameters)
    fill = {SPRING2D: (NAN, NAN), BOUNCE2D: (SENTINEL, SENTINEL)}[cell] if prefill is None else prefill
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
    if cell == BOUNCE2D:
        pos0, vel0, rep = C2.bouncing_overshoot_inputs(B, R) if kind == "overshoot" else C2.bouncing_inputs(B, R)
    else:
        pos0, vel0, rep = C2.spring_inputs(B, R, seed=SPRING_SEED.get((B, R), 0))
    dr, dv = C.adjoints(B, R, D, 31 * B + R)
    return (pos0, vel0, rep, dr, dv) + C2.reference(cell, pos0, vel0, R, dr, dv)


def _judge(what, got, f64, f32, keys):
    """Print and assert the envelope bars of ``keys``."""
    bad = []
    for k, (e, e32, bar) in C.envelope_rows(got, f64, f32, keys).items():
        print(f"ENVELOPE {what:34s} {k:6s} kernel {e:.2e}  e32 {e32:.2e}  bar {bar:.2e}")
        assert bar <= C.NORTH_STAR, f"{what}: the inputs put the {k} bar at {bar:.2e} > 1e-4"
        if not e <= bar:
            bad.append(f"{k}: {e:.3e} > {bar:.3e}")
    assert not bad, f"{what}: {bad}"


# ------------------------------------------------------------------ spring ----
@pytest.mark.parametrize("B,R", [(1, 1), (65, 6), (130, 20), (37, 65)])
def test_spring2d(B, R):
    """Two objects 6-14 px apart at random angles, |v| <= 8, k = log 2,
    equil = log 3; the float64 replay keeps n >= 1 at every substep.  65 and
    130 sequences: two and three partial rows of the serial adjoint; R = 65:
    past the 1-D spring's scan (the serial adjoint is the only backward here)."""
    pos0, vel0, rep, dr, dv, f64, f32 = _case(SPRING2D, "spring", B, R)
    flips = (rep["flips"] > 0).sum(0).tolist()
    print(f"spring 2-D B={B} R={R}: n >= {float(rep['nmin'].min()):.2f}, sequences whose d_x / d_y change sign {flips}")
    assert float(rep["nmin"].min()) >= 1.0, "the spring passes n < 1: d / (n + 1e-4) decorrelates any fp32 run"
    if R >= 6:
        assert min(flips) >= 1, "d_x and d_y must each change sign in at least one sequence"
    got = hip_rollout(SPRING2D, pos0, vel0, R, dr, dv)
    # object 1 (columns 2, 3) moves
    assert float(np.abs(got["pvs"][:, R, 2:4] - got["pvs"][:, 0, 2:4]).min()) > 0
    _judge(f"spring 2-D B={B} R={R}", got, f64, f32, ("pvs",) + GRAD_KEYS[SPRING2D])


# ---------------------------------------------------------------- bouncing ----
def _bouncing_checks(got, f64):
    """Velocities only ever change sign: bit-equal to the float64 replay's +-vel0."""
    assert np.array_equal(got["pvs"][:, :, 4:], f64["pvs"][:, :, 4:]), "a velocity is not +-vel0 as in the float64 replay"


@pytest.mark.parametrize("B,R", [(1, 1), (65, 6), (130, 20), (5, 96)])
def test_bouncing2d_walls(B, R):
    """rollout_cases.bouncing_inputs' recipe on all four columns (pos0 ~
    U[4, 28], vel0 ~ U[-40, 40]): 3 flag bits x 4 coordinates per substep;
    R = 96: bench's longest rollout."""
    pos0, vel0, rep, dr, dv, f64, f32 = _case(BOUNCE2D, "walls", B, R)
    hits = torch.stack([rep["up"].sum(0), rep["low"].sum(0)])      # [wall, column]
    print(f"bouncing 2-D B={B} R={R}: upper-wall hits {hits[0].tolist()}, lower-wall hits {hits[1].tolist()}, "
          f"margin {float(rep['margin'].min()):.2e}")
    assert float(rep["margin"].min()) >= C.BOUNCE_MARGIN
    if R >= 20:
        assert int(hits.min()) >= 1, f"a column never hits a wall: {hits.tolist()}"
    got = hip_rollout(BOUNCE2D, pos0, vel0, R, dr, dv)
    _bouncing_checks(got, f64)
    assert got["g0"][0] == SENTINEL and got["g1"][0] == SENTINEL, "bouncing has no parameters to write"
    _judge(f"bouncing 2-D B={B} R={R}", got, f64, f32, ("pvs",) + GRAD_KEYS[BOUNCE2D])


def test_bouncing2d_overshoot():
    """|vel0[:, 2]| > 480 (object 1's x): a substep overshoots the far wall so
    far that the reflected position lies beyond the near wall (flags a and c
    together, bits 6 and 8 of the 12)."""
    pos0, vel0, rep, dr, dv, f64, f32 = _case(BOUNCE2D, "overshoot", 8, 2)
    assert bool((vel0[:, 2].abs() > 480).all()) and bool((rep["ac"][:, 2] >= 1).all()), rep["ac"].tolist()
    got = hip_rollout(BOUNCE2D, pos0, vel0, 2, dr, dv)
    _bouncing_checks(got, f64)
    _judge("bouncing 2-D overshoot B=8 R=2", got, f64, f32, ("pvs",) + GRAD_KEYS[BOUNCE2D])


# ---------------------------------------------------------- argument forms ----
FORM_R = {SPRING2D: 3, BOUNCE2D: 4}
FORMS = ("null_vel0", "pos0_ld", "null_dpos_roll", "null_dpvs", "null_dvel0", "accumulate")


@functools.lru_cache(maxsize=None)
def _form_reference(cell, form):
    B, R = 65, FORM_R[cell]
    pick = C2.bouncing_inputs if cell == BOUNCE2D else C2.spring_inputs
    # (null vel0: the picker replays the inputs as this form runs them, at rest)
    pos0, vel0, rep = pick(B, R, seed=9, zero_vel=form == "null_vel0")
    assert float(rep["nmin" if cell == SPRING2D else "margin"].min()) >= (1.0 if cell == SPRING2D else C.BOUNCE_MARGIN)
    dr, dv = C.adjoints(B, R, D, 18)
    if form == "null_dpos_roll":
        dr = None
    if form == "null_dpvs":
        dv = None
    return (pos0, vel0, dr, dv) + C2.reference(cell, pos0, vel0, R, dr, dv)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cell", [SPRING2D, BOUNCE2D])
def test_argument_forms_2d(cell, form):
    """Every argument form the engine and the module path take, at B = 65
    (two partial rows), against the float64 reference with the corresponding
    term dropped."""
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
        for i, fill in enumerate(kw["prefill"]):
            if cell == SPRING2D:
                got[f"g{i}"] = got[f"g{i}"] - fill
            else:
                assert got[f"g{i}"][0] == fill, f"gparam{i} touched"
    elif cell == BOUNCE2D:
        assert got["g0"][0] == SENTINEL and got["g1"][0] == SENTINEL
    _judge(f"{NAME[cell]} {form}", got, f64, f32, keys)


def test_unsupported_and_missing_parameters_2d():
    """Argument checks that return before any launch: the new kinds have no
    D = 6 kernel (PAIG_E_UNSUPPORTED, with a message); kind 3 without its
    parameters is PAIG_E_SHAPE; nothing is written."""
    lib = L()
    fwd, bwd = lib.fns["paig_rollout_fwd"], lib.fns["paig_rollout_bwd"]
    B, R = 3, 2
    dt = C2.cell_dt().to(DEV)
    q = torch.zeros(2, dtype=torch.float64, device=DEV)
    for cell, D_ in ((SPRING2D, 6), (BOUNCE2D, 6)):
        pos0, vel0 = torch.full((B, D_), 16.0, device=DEV), torch.zeros(D_ // 2, B, 2, device=DEV)
        pvs = torch.full((B, R + 1, 2 * D_), NAN, device=DEV)
        rc = fwd(cell, p_(pos0), D_, p_(vel0), p_(dt), p_(q), p_(q) + 8, p_(pvs), B, D_, R, st())
        assert rc == PAIG_E_UNSUPPORTED, rc
        msg = lib.paig_last_error().decode()
        assert "unsupported" in msg and f"D={D_}" in msg, msg
        dpos0 = torch.full((B, D_), NAN, device=DEV)
        part = torch.full((2 * lib.paig_rollout_bwd_blocks(B),), NAN, device=DEV, dtype=torch.float64)
        rc = bwd(cell, p_(pvs), None, None, p_(dt), p_(q), p_(q) + 8, p_(dpos0), None, p_(part), p_(q), p_(q) + 8, 0,
                 B, D_, R, st())
        assert rc == PAIG_E_UNSUPPORTED, rc
        assert f"D={D_}" in lib.paig_last_error().decode()
        torch.cuda.synchronize()
        assert bool(torch.isnan(pvs).all()) and bool(torch.isnan(dpos0).all()) and bool(torch.isnan(part).all())
    pos0 = torch.full((B, D), 16.0, device=DEV)
    pvs = torch.full((B, R + 1, 2 * D), NAN, device=DEV)
    rc = fwd(SPRING2D, p_(pos0), D, None, p_(dt), None, p_(q) + 8, p_(pvs), B, D, R, st())
    assert rc == PAIG_E_SHAPE, rc
    assert "physics params required" in lib.paig_last_error().decode()
    dpos0 = torch.full((B, D), NAN, device=DEV)
    part = torch.full((2 * lib.paig_rollout_bwd_blocks(B),), NAN, device=DEV, dtype=torch.float64)
    rc = bwd(SPRING2D, p_(pvs), None, None, p_(dt), None, p_(q) + 8, p_(dpos0), None, p_(part), p_(q), p_(q) + 8, 0,
             B, D, R, st())
    assert rc == PAIG_E_SHAPE, rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(pvs).all()) and bool(torch.isnan(dpos0).all()) and bool(torch.isnan(part).all())
    assert bool((q == 0).all())
