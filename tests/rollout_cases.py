"""Inputs and references for the direct tests of the rollout cells
(csrc/rollout.hip, csrc/rollout_cells.h): states at which the bouncing walls
and the gravity clamps act, chosen by a float64 CPU replay alone.

Every recipe draws 2 B candidates with a fixed seed, replays them in float64
and keeps the first B whose branch decisions sit a margin away from their
thresholds (an honest fp32 run then takes the same branches); a recipe that
would have to discard more than half of its candidates fails.  The replays
restate the oracle's cells substep by substep (the oracle shows only whole
steps) and are held to the oracle's float64 result bit for bit.

The reference of a case is autograd through the oracle's cell applied R
times, in float64; its fp32 ensemble (the same code in fp32, and on pos0 /
vel0 perturbed by at most one ulp) gives the error an honest fp32
implementation makes: tests/envelope.py's rule.
"""
import functools
import math

import numpy as np
import torch

from envelope import ENVELOPE_FLOOR, ENVELOPE_K, _ulp_perturbed
from helpers import rel_err
from oracle import physics_oracle as O

SPRING, BOUNCE, GRAVITY = 0, 1, 2
CELL_FN = {SPRING: O.spring_cell, BOUNCE: O.bouncing_cell, GRAVITY: O.gravity_cell}
CELL_D = {SPRING: 4, BOUNCE: 4, GRAVITY: 6}
CELL_DT = {SPRING: 0.3, BOUNCE: 0.3, GRAVITY: 0.5}
ENSEMBLE = 5                      # one-ulp perturbations of (pos0, vel0) beside the plain fp32 run
NORTH_STAR = 1e-4
BOUNCE_MARGIN = 5e-3              # px: about 15x the worst fp32 position error at R = 70
BOUNCE_FIXED = (40.0, -3.0)       # columns 2, 3: outside the walls, never moved (split-size-1 quirk)
GRAV_MARGIN = 0.01                # relative distance of sq / nrm from the clamp thresholds
GRAV_FREE_MIN = 3.0               # px: closest approach of a free-regime pair
REGIMES = ("touching", "near", "free", "far", "veryfar")


def f32_param(x):
    """A physics parameter that fp32 holds exactly, as the float64 the kernels read."""
    return torch.tensor(float(np.float32(x)), dtype=torch.float64)


def default_params(cell):
    if cell == SPRING:
        return {"k": f32_param(math.log(4.0)), "equil": f32_param(math.log(3.0))}
    if cell == GRAVITY:
        return {"g": f32_param(math.log(3.0)), "m": f32_param(math.log(1.5))}
    return {}


def cell_dt(cell):
    return torch.tensor(CELL_DT[cell], dtype=torch.float32)


def _oracle_P(cell, dt, prm, dtype, leaves=True):
    P = {"rollout_cell.dt": dt.to(dtype)}
    for k, v in prm.items():
        v = v.detach().to(dtype).clone()
        P["rollout_cell." + k] = v.requires_grad_(True) if leaves and k != "m" else v
    return P


def _oracle_steps(cell, pos0, vel0, dt, prm, R):
    """float64 oracle states after each of R steps (no autograd): ([R, B, D], [R, B, D])."""
    P = _oracle_P(cell, dt, prm, torch.float64, leaves=False)
    p, v = pos0.double(), vel0.double()
    ps, vs = [], []
    with torch.no_grad():
        for _ in range(R):
            p, v = CELL_FN[cell](P, p, v)
            ps.append(p)
            vs.append(v)
    return torch.stack(ps), torch.stack(vs)


# ---------------------------------------------------------------- bouncing ----
def bounce_replay(pos0, vel0, R, dt):
    """float64 replay of bouncing_cell, substep by substep, for columns 0, 1.
    Returns per sequence: margin (the closest any wall comparison came to its
    threshold, px), up / low (hits of the upper / lower wall per column,
    [B, 2]) and ac (substeps in which the upper reflection landed beyond the
    lower wall: flags a and c together, column 0)."""
    h = dt.double() / 5
    p, v = pos0.double()[:, :2].clone(), vel0.double()[:, :2].clone()
    B = p.shape[0]
    margin = torch.full((B,), float("inf"), dtype=torch.float64)
    up, low = torch.zeros(B, 2, dtype=torch.long), torch.zeros(B, 2, dtype=torch.long)
    ac = torch.zeros(B, dtype=torch.long)
    ends_p, ends_v = [], []
    for _ in range(R):
        for _ in range(5):
            p = p + h * v
            a = p + 2 > 32
            b = 0.0 > p - 2
            margin = torch.minimum(margin, torch.minimum((p + 2 - 32).abs(), (p - 2).abs()).amin(1))
            v = torch.where(a, -v, v)
            v = torch.where(b, -v, v)
            p = torch.where(a, 32 - (p + 2 - 32) - 2, p)
            c = 0.0 > p - 2
            margin = torch.minimum(margin, (p - 2).abs().amin(1))
            p = torch.where(c, -(p - 2) + 2, p)
            up += a
            low += b | c
            ac += a[:, 0] & c[:, 0]
        ends_p.append(p)
        ends_v.append(v)
    return {"margin": margin, "up": up, "low": low, "ac": ac, "pos": torch.stack(ends_p), "vel": torch.stack(ends_v)}


def _keep_first(ok, B, what):
    idx = torch.nonzero(ok).flatten()
    assert len(idx) >= B, f"{what}: only {len(idx)} of {len(ok)} candidates keep the margin (need {B}: at most half may go)"
    return idx[:B]


def _bounce_pick(pos0, vel0, B, R, what):
    dt = cell_dt(BOUNCE)
    keep = _keep_first(bounce_replay(pos0, vel0, R, dt)["margin"] >= BOUNCE_MARGIN, B, what)
    pos0, vel0 = pos0[keep].contiguous(), vel0[keep].contiguous()
    rep = bounce_replay(pos0, vel0, R, dt)
    # the replay is the oracle's cell: same float64 states after every step
    op, ov = _oracle_steps(BOUNCE, pos0, vel0, dt, {}, R)
    assert torch.equal(rep["pos"], op[:, :, :2]) and torch.equal(rep["vel"], ov[:, :, :2]), what
    assert bool((rep["margin"] >= BOUNCE_MARGIN).all()), what
    return pos0, vel0, rep


@functools.lru_cache(maxsize=None)
def bouncing_inputs(B, R, seed=0):
    """(pos0, vel0 [B, 4] fp32, replay): columns 0, 1 ~ U[4, 28] / U[-40, 40]."""
    g = torch.Generator().manual_seed(1000 * R + B + seed)
    n = 2 * B
    pos0 = torch.empty(n, 4)
    vel0 = torch.zeros(n, 4)
    pos0[:, :2] = 4 + 24 * torch.rand(n, 2, generator=g)
    vel0[:, :2] = 80 * torch.rand(n, 2, generator=g) - 40
    pos0[:, 2], pos0[:, 3] = BOUNCE_FIXED
    vel0[:, 2:] = torch.rand(n, 2, generator=g) - 0.5
    return _bounce_pick(pos0, vel0, B, R, f"bouncing B={B} R={R}")


@functools.lru_cache(maxsize=None)
def bouncing_overshoot_inputs(B=8, R=2, seed=0):
    """|vel0[:, 0]| in [950, 1200]: one substep carries column 0 so far past
    the far wall that its reflection lies beyond the near wall (h |v| >= 57
    px on a 28 px court), either in the first substep (v > 0) or in the second
    (v < 0, after the lower wall's own reflection)."""
    g = torch.Generator().manual_seed(77 + seed)
    pos0, vel0, _ = bouncing_inputs(2 * B, R, seed=5)
    pos0, vel0 = pos0.clone(), vel0.clone()
    mag = 950 + 250 * torch.rand(2 * B, generator=g)
    vel0[:, 0] = torch.where(torch.arange(2 * B) % 2 == 0, mag, -mag)
    pos0, vel0, rep = _bounce_pick(pos0, vel0, B, R, "bouncing overshoot")
    assert bool((vel0[:, 0].abs() > 480).all()) and bool((rep["ac"] >= 1).all())
    return pos0, vel0, rep


def bouncing_wall_states(n):
    """n states whose single step (R = 1) hits a wall, in recipe order."""
    pos0, vel0, rep = bouncing_inputs(8 * n, 1, seed=3)
    idx = torch.nonzero((rep["up"] + rep["low"]).sum(1) > 0).flatten()
    assert len(idx) >= n, len(idx)
    idx = idx[:n]
    return pos0[idx].contiguous(), vel0[idx].contiguous()


# ----------------------------------------------------------------- gravity ----
def gravity_replay(pos0, vel0, R, dt, prm):
    """float64 replay of gravity_cell, substep by substep.  Per sequence:
    counts [B, 5] of pair-substeps in each regime (REGIMES), margin (the
    smallest relative distance of any pair's sq / nrm from 0.1, 1e5 / 1, 170)
    and dmin (the closest approach of any pair, px)."""
    h = dt.double() / 5
    A = torch.exp(prm["g"].double()) * torch.exp(2 * prm["m"].double())
    p, v = pos0.double().clone(), vel0.double().clone()
    B = p.shape[0]
    counts = torch.zeros(B, 5, dtype=torch.long)
    margin = torch.full((B,), float("inf"), dtype=torch.float64)
    dmin = torch.full((B,), float("inf"), dtype=torch.float64)
    ends_p, ends_v = [], []
    for _ in range(R):
        for _ in range(5):
            vecs = [p[:, 0:2] - p[:, 2:4], p[:, 2:4] - p[:, 4:6], p[:, 4:6] - p[:, 0:2]]
            Fs = []
            for vec in vecs:
                sq = torch.sum(vec ** 2, dim=-1, keepdim=True)
                nrm = torch.sqrt(torch.clamp(sq, min=1e-1, max=1e5))
                Fs.append(vec / torch.pow(torch.clamp(nrm, min=1, max=170), 3))
                s, n = sq[:, 0], nrm[:, 0]
                reg = torch.where(s < 0.1, 0, torch.where(n < 1, 1, torch.where(n <= 170, 2, torch.where(s <= 1e5, 3, 4))))
                counts += torch.nn.functional.one_hot(reg, 5)
                rel = torch.stack([(s / 0.1 - 1).abs(), (s / 1e5 - 1).abs(), (n - 1).abs(), (n / 170 - 1).abs()]).amin(0)
                margin = torch.minimum(margin, rel)
                dmin = torch.minimum(dmin, torch.sqrt(s))
            Fs = [Fs[0] - Fs[2], Fs[1] - Fs[0], Fs[2] - Fs[1]]
            Fs = torch.cat([-A * f for f in Fs], 1)
            v = v + h * Fs
            p = p + h * v
        ends_p.append(p)
        ends_v.append(v)
    return {"counts": counts, "margin": margin, "dmin": dmin, "pos": torch.stack(ends_p), "vel": torch.stack(ends_v)}


def _unit(theta):
    return torch.stack([torch.cos(theta), torch.sin(theta)], -1)


def _gravity_candidates(group, n, g):
    c = torch.tensor([18.0, 18.0])
    if group == "free":
        # a ring of radius 4..10 px around (18, 18), angles 120 degrees apart +- 0.2 rad
        th0 = 2 * math.pi * torch.rand(n, 1, generator=g)
        th = th0 + torch.arange(3) * (2 * math.pi / 3) + 0.4 * (torch.rand(n, 3, generator=g) - 0.5)
        r = 4 + 6 * torch.rand(n, 3, generator=g)
        pos0 = (c + r[..., None] * _unit(th)).reshape(n, 6)
    else:
        lo, hi = {"near": (0.6, 0.66), "touching": (0.2, 0.22), "far": (220.0, 242.0), "veryfar": (400.0, 440.0)}[group]
        d = lo + (hi - lo) * torch.rand(n, generator=g)
        b0 = c + 2 * (torch.rand(n, 2, generator=g) - 0.5)
        b1 = b0 + d[:, None] * _unit(2 * math.pi * torch.rand(n, generator=g))
        b2 = b0 + (11 + torch.rand(n, 1, generator=g)) * _unit(2 * math.pi * torch.rand(n, generator=g))
        pos0 = torch.cat([b0, b1, b2], 1)
    vel0 = torch.rand(n, 6, generator=g) - 0.5
    return pos0, vel0


@functools.lru_cache(maxsize=None)
def gravity_inputs(group, B, R, seed=0):
    """(pos0, vel0 [B, 6] fp32, replay) of one regime group."""
    dt, prm = cell_dt(GRAVITY), default_params(GRAVITY)
    g = torch.Generator().manual_seed(REGIMES.index(group) * 100003 + 1000 * R + B + seed)
    pos0, vel0 = _gravity_candidates(group, 2 * B, g)
    own = REGIMES.index(group)

    def ok(rep):
        if group == "free":
            return (rep["dmin"] >= GRAV_FREE_MIN) & (rep["counts"][:, own] == 15 * R)
        return (rep["margin"] >= GRAV_MARGIN) & (rep["counts"][:, own] > 0)
    what = f"gravity {group} B={B} R={R}"
    keep = _keep_first(ok(gravity_replay(pos0, vel0, R, dt, prm)), B, what)
    pos0, vel0 = pos0[keep].contiguous(), vel0[keep].contiguous()
    rep = gravity_replay(pos0, vel0, R, dt, prm)
    op, ov = _oracle_steps(GRAVITY, pos0, vel0, dt, prm, R)
    assert torch.equal(rep["pos"], op) and torch.equal(rep["vel"], ov), what
    assert bool(ok(rep).all()) and int(rep["counts"][:, own].sum()) > 0, what
    return pos0, vel0, rep


def assert_margins(cell, pos0, vel0, R, group=None, prm=None, dt=None):
    """The margin rule on the inputs a test really uses (an argument form may
    change them: no initial velocity, a fixture's parameters); returns the replay."""
    dt = cell_dt(cell) if dt is None else dt
    if cell == BOUNCE:
        rep = bounce_replay(pos0, vel0, R, dt)
        assert bool((rep["margin"] >= BOUNCE_MARGIN).all()), float(rep["margin"].min())
    else:
        rep = gravity_replay(pos0, vel0, R, dt, default_params(GRAVITY) if prm is None else prm)
        if group == "free":
            assert bool((rep["dmin"] >= GRAV_FREE_MIN).all()), float(rep["dmin"].min())
            assert bool((rep["counts"][:, 2] == 15 * R).all())
        else:
            assert bool((rep["margin"] >= GRAV_MARGIN).all()), float(rep["margin"].min())
    return rep


# ------------------------------------------------------------------ spring ----
@functools.lru_cache(maxsize=None)
def spring_inputs(B, R, seed=None):
    """test_rollout_spring_adjoint_scan_and_serial's recipe, adjoints included
    (pos0, vel0, dpos_roll, dpvs): the spring's ends (columns 0, 1) near the
    rest length 6, so the oscillation never passes n = 0 where
    d / (n + 1e-4) has a 1e4 slope."""
    g = torch.Generator().manual_seed(R if seed is None else seed)
    pos0 = 16 + 2 * (torch.rand(B, 4, generator=g) - 0.5)
    sgn = torch.where(torch.rand(B, generator=g) < 0.5, -1.0, 1.0)
    pos0[:, 0] = pos0[:, 1] + sgn * (6 + 2 * (torch.rand(B, generator=g) - 0.5))
    vel0 = torch.rand(B, 4, generator=g) - 0.5
    return pos0, vel0, torch.randn(B, R, 4, generator=g), torch.randn(B, R + 1, 8, generator=g)


# --------------------------------------------------------------- reference ----
def adjoints(B, R, D, seed):
    """The spring test's loss: random adjoints of every step's positions
    (dpos_roll [B, R, D]) and of the whole pos_vel_seq (dpvs [B, R+1, 2D])."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, R, D, generator=g), torch.randn(B, R + 1, 2 * D, generator=g)


def oracle_run(cell, pos0, vel0, R, dpos_roll, dpvs, dtype, prm=None, dt=None):
    """Autograd through the oracle's cell applied R times, in ``dtype``:
    {pvs [B, R+1, 2D], dpos0, dvel0 [B, D], g0, g1} as float64 numpy."""
    D = CELL_D[cell]
    prm = default_params(cell) if prm is None else prm
    dt = cell_dt(cell) if dt is None else dt
    P = _oracle_P(cell, dt, prm, dtype)
    p = pos0.to(dtype).clone().requires_grad_(True)
    v = vel0.to(dtype).clone().requires_grad_(True)
    loss = (p * 0).sum() + (v * 0).sum()
    if dpvs is not None:
        loss = loss + (dpvs[:, 0, :D].to(dtype) * p).sum() + (dpvs[:, 0, D:].to(dtype) * v).sum()
    pc, vc = p, v
    ps, vs = [p], [v]
    for t in range(R):
        pc, vc = CELL_FN[cell](P, pc, vc)
        ps.append(pc)
        vs.append(vc)
        if dpos_roll is not None:
            loss = loss + (dpos_roll[:, t].to(dtype) * pc).sum()
        if dpvs is not None:
            loss = loss + (dpvs[:, t + 1, :D].to(dtype) * pc).sum() + (dpvs[:, t + 1, D:].to(dtype) * vc).sum()
    loss.backward()
    out = {"pvs": torch.cat([torch.stack(ps, 1), torch.stack(vs, 1)], 2), "dpos0": p.grad, "dvel0": v.grad}
    names = {SPRING: ("k", "equil"), GRAVITY: ("g",), BOUNCE: ()}[cell]
    for i, k in enumerate(names):
        out[f"g{i}"] = P["rollout_cell." + k].grad.reshape(1)
    return {k: t.detach().double().numpy() for k, t in out.items()}


def reference(cell, pos0, vel0, R, dpos_roll, dpvs, prm=None, dt=None):
    """(float64 result, [fp32 result, fp32 results on one-ulp-perturbed pos0 / vel0])."""
    f64 = oracle_run(cell, pos0, vel0, R, dpos_roll, dpvs, torch.float64, prm, dt)
    f32 = [oracle_run(cell, pos0, vel0, R, dpos_roll, dpvs, torch.float32, prm, dt)]
    for s in range(ENSEMBLE):
        q = _ulp_perturbed({"pos0": pos0, "vel0": vel0}, s)
        f32.append(oracle_run(cell, q["pos0"], q["vel0"], R, dpos_roll, dpvs, torch.float32, prm, dt))
    return f64, f32


def envelope_rows(got, f64, f32, keys, rows=None):
    """{key: (error of ``got``, e32, bar)}: normwise distances to float64 over
    the sequences ``rows`` (one regime group; all when None); e32 is the
    furthest fp32 ensemble member, bar = max(ENVELOPE_K e32, ENVELOPE_FLOOR)."""
    def sl(k, a):
        return a if rows is None or k in ("g0", "g1") else a[rows]   # (a parameter gradient is the batch's)
    out = {}
    for k in keys:
        e32 = max(rel_err(sl(k, r[k]), sl(k, f64[k])) for r in f32)
        out[k] = (rel_err(sl(k, np.asarray(got[k])), sl(k, f64[k])), e32, max(ENVELOPE_K * e32, ENVELOPE_FLOOR))
    return out
