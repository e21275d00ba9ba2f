"""Inputs and references for the tests of the opt-in 2-D rollout cells
(spring2d_ode_cell / bouncing2d_ode_cell, paig_rollout_fwd/bwd kinds 3 / 4).

The reference is a torch restatement of the spring and bouncing cells with
the split size as an argument: split 1 is the reference's behaviour (objects
"0" and "1" are the columns x0, y0: quirk Q3, held bit for bit to
oracle.physics_oracle in tests/test_rollout2d_ref_cpu.py), split 2 the two
objects (x0, y0), (x1, y1) in the plane.  It runs in float64 (the truth) and in
fp32 (the ensemble of tests/envelope.py's rule), under autograd.

The input pickers draw candidates with a fixed seed, replay them in float64
substep by substep and keep the first B whose decisions sit a margin away from
their thresholds (spring: n >= 1 at every substep; bouncing: every wall
comparison >= BOUNCE_MARGIN from its threshold).  At most 3 of every 4
candidates may be discarded.
"""
import functools
import math

import torch

from envelope import _ulp_perturbed
from rollout_cases import BOUNCE_MARGIN, ENSEMBLE, _oracle_P, adjoints, f32_param  # noqa: F401  (adjoints: re-exported)

SPRING2D, BOUNCE2D = 3, 4
D = 4
DT = 0.3
CANDIDATES = 4                    # candidates drawn per kept sequence
SPRING_NMIN = 1.0                 # px: the spring never comes closer to n = 0 (the 1-D test's condition)


def cell_dt():
    return torch.tensor(DT, dtype=torch.float32)


def spring_params():
    """Non-default k, equil that fp32 holds exactly: exp(k) = 2, rest length 2 exp(equil) = 6 px."""
    return {"k": f32_param(math.log(2.0)), "equil": f32_param(math.log(3.0))}


# ------------------------------------------------------------ the two cells ----
def spring_cell(P, pos, vel, split=2):
    """One step (5 substeps of dt / 5) of the spring cell; objects 0 and 1 are
    the first two chunks of width ``split`` of pos / vel."""
    dt, k, eq = P["rollout_cell.dt"], P["rollout_cell.k"], P["rollout_cell.equil"]
    p, v = list(torch.split(pos, split, 1)), list(torch.split(vel, split, 1))
    for _ in range(5):
        n = torch.sqrt(torch.abs(torch.sum((p[0] - p[1]) ** 2, dim=-1, keepdim=True)))
        d = (p[0] - p[1]) / (n + 1e-4)
        Fs = torch.exp(k) * (n - 2 * torch.exp(eq)) * d
        v[0] = v[0] - dt / 5 * Fs
        v[1] = v[1] + dt / 5 * Fs
        p[0] = p[0] + dt / 5 * v[0]
        p[1] = p[1] + dt / 5 * v[1]
    return torch.cat(p, 1), torch.cat(v, 1)


def bouncing_cell(P, pos, vel, split=2):
    """One step of the bouncing cell (walls 0 and 32, radius 2) on the first
    two chunks of width ``split``."""
    dt = P["rollout_cell.dt"]
    p, v = list(torch.split(pos, split, 1)), list(torch.split(vel, split, 1))
    for _ in range(5):
        p[0] = p[0] + dt / 5 * v[0]
        p[1] = p[1] + dt / 5 * v[1]
        for j in range(2):
            v[j] = torch.where(p[j] + 2 > 32, -v[j], v[j])
            v[j] = torch.where(0.0 > p[j] - 2, -v[j], v[j])
            p[j] = torch.where(p[j] + 2 > 32, 32 - (p[j] + 2 - 32) - 2, p[j])
            p[j] = torch.where(0.0 > p[j] - 2, -(p[j] - 2) + 2, p[j])
    return torch.cat(p, 1), torch.cat(v, 1)


CELL_FN = {SPRING2D: spring_cell, BOUNCE2D: bouncing_cell}
PARAM_NAMES = {SPRING2D: ("k", "equil"), BOUNCE2D: ()}


def default_params(cell):
    return spring_params() if cell == SPRING2D else {}


def cell_steps(cell, pos0, vel0, R, prm, split=2):
    """float64 states after each of R steps of the restated cell (no autograd): ([R, B, D], [R, B, D])."""
    P = _oracle_P(0, cell_dt(), prm, torch.float64, leaves=False)
    p, v = pos0.double(), vel0.double()
    ps, vs = [], []
    with torch.no_grad():
        for _ in range(R):
            p, v = CELL_FN[cell](P, p, v, split)
            ps.append(p)
            vs.append(v)
    return torch.stack(ps), torch.stack(vs)


# --------------------------------------------------------------- reference ----
def run(cell, pos0, vel0, R, dpos_roll, dpvs, dtype, prm=None, split=2):
    """Autograd through the restated cell applied R times, in ``dtype``, with
    rollout_cases' loss (random adjoints of every step's positions and of the
    whole pos_vel_seq): {pvs [B, R+1, 2D], dpos0, dvel0 [B, D], g0, g1} as float64 numpy."""
    prm = default_params(cell) if prm is None else prm
    P = _oracle_P(0, cell_dt(), prm, dtype)
    p = pos0.to(dtype).clone().requires_grad_(True)
    v = vel0.to(dtype).clone().requires_grad_(True)
    loss = (p * 0).sum() + (v * 0).sum()
    if dpvs is not None:
        loss = loss + (dpvs[:, 0, :D].to(dtype) * p).sum() + (dpvs[:, 0, D:].to(dtype) * v).sum()
    pc, vc = p, v
    ps, vs = [p], [v]
    for t in range(R):
        pc, vc = CELL_FN[cell](P, pc, vc, split)
        ps.append(pc)
        vs.append(vc)
        if dpos_roll is not None:
            loss = loss + (dpos_roll[:, t].to(dtype) * pc).sum()
        if dpvs is not None:
            loss = loss + (dpvs[:, t + 1, :D].to(dtype) * pc).sum() + (dpvs[:, t + 1, D:].to(dtype) * vc).sum()
    loss.backward()
    out = {"pvs": torch.cat([torch.stack(ps, 1), torch.stack(vs, 1)], 2), "dpos0": p.grad, "dvel0": v.grad}
    for i, k in enumerate(PARAM_NAMES[cell]):
        g = P["rollout_cell." + k].grad
        out[f"g{i}"] = (torch.zeros(1, dtype=dtype) if g is None else g.reshape(1))
    return {k: t.detach().double().numpy() for k, t in out.items()}


def reference(cell, pos0, vel0, R, dpos_roll, dpvs, prm=None):
    """(float64 result, [fp32 result, fp32 results on one-ulp-perturbed pos0 / vel0])."""
    f64 = run(cell, pos0, vel0, R, dpos_roll, dpvs, torch.float64, prm)
    f32 = [run(cell, pos0, vel0, R, dpos_roll, dpvs, torch.float32, prm)]
    for s in range(ENSEMBLE):
        q = _ulp_perturbed({"pos0": pos0, "vel0": vel0}, s)
        f32.append(run(cell, q["pos0"], q["vel0"], R, dpos_roll, dpvs, torch.float32, prm))
    return f64, f32


def _keep_first(ok, B, what):
    idx = torch.nonzero(ok).flatten()
    assert len(idx) >= B and 4 * (len(ok) - len(idx)) <= 3 * len(ok), \
        f"{what}: {len(idx)} of {len(ok)} candidates keep the margin (need {B}: at most 3 of every 4 may go)"
    return idx[:B]


# ------------------------------------------------------------------ spring ----
def spring_replay(pos0, vel0, R, prm):
    """float64 replay of the 2-D spring, substep by substep.  Per sequence:
    nmin (the smallest n = |p0 - p1| entering any substep) and flips [B, 2]
    (sign changes of d_x, d_y over the substeps); pos / vel: states after each step."""
    h = cell_dt().double() / 5
    ek, tee = torch.exp(prm["k"].double()), 2 * torch.exp(prm["equil"].double())
    p, v = pos0.double().clone(), vel0.double().clone()
    B = p.shape[0]
    nmin = torch.full((B,), float("inf"), dtype=torch.float64)
    flips = torch.zeros(B, 2, dtype=torch.long)
    ends_p, ends_v = [], []
    sign = torch.sign(p[:, 0:2] - p[:, 2:4])
    for _ in range(R):
        for _ in range(5):
            d = p[:, 0:2] - p[:, 2:4]
            n = torch.sqrt(torch.abs(torch.sum(d ** 2, dim=-1, keepdim=True)))
            nmin = torch.minimum(nmin, n[:, 0])
            s = torch.sign(d)
            flips += (s * sign < 0)
            sign = torch.where(s != 0, s, sign)
            Fs = ek * (n - tee) * (d / (n + 1e-4))
            v0 = v[:, 0:2] - h * Fs
            v1 = v[:, 2:4] + h * Fs
            p = torch.cat([p[:, 0:2] + h * v0, p[:, 2:4] + h * v1], 1)
            v = torch.cat([v0, v1], 1)
        ends_p.append(p)
        ends_v.append(v)
    return {"nmin": nmin, "flips": flips, "pos": torch.stack(ends_p), "vel": torch.stack(ends_v)}


def _unit(theta):
    return torch.stack([torch.cos(theta), torch.sin(theta)], -1)


@functools.lru_cache(maxsize=None)
def spring_inputs(B, R, seed=0, zero_vel=False):
    """(pos0, vel0 [B, 4] fp32, replay): the two objects 6-14 px apart at a
    random angle around (16, 16) +- 2, each with |v| <= 8 at a random angle
    (zero_vel: at rest, the null-vel0 argument form), kept where the float64
    replay has n >= SPRING_NMIN at every substep."""
    prm = spring_params()
    g = torch.Generator().manual_seed(7000 * R + B + seed)
    n = CANDIDATES * B
    c = 16 + 4 * (torch.rand(n, 2, generator=g) - 0.5)
    half = (3 + 4 * torch.rand(n, 1, generator=g)) * _unit(2 * math.pi * torch.rand(n, generator=g))
    pos0 = torch.cat([c + half, c - half], 1)
    vel0 = torch.cat([8 * torch.rand(n, 1, generator=g) * _unit(2 * math.pi * torch.rand(n, generator=g))
                      for _ in range(2)], 1)
    if zero_vel:
        vel0 = torch.zeros_like(vel0)
    what = f"spring 2-D B={B} R={R}"
    keep = _keep_first(spring_replay(pos0, vel0, R, prm)["nmin"] >= SPRING_NMIN, B, what)
    pos0, vel0 = pos0[keep].contiguous(), vel0[keep].contiguous()
    rep = spring_replay(pos0, vel0, R, prm)
    # the replay is the restated cell: the same float64 states after every step
    op, ov = cell_steps(SPRING2D, pos0, vel0, R, prm)
    assert torch.equal(rep["pos"], op) and torch.equal(rep["vel"], ov), what
    sep = (pos0[:, 0:2] - pos0[:, 2:4]).norm(dim=1)
    assert float(sep.min()) >= 6 - 1e-4 and float(sep.max()) <= 14 + 1e-4
    assert float(vel0[:, 0:2].norm(dim=1).max()) <= 8 + 1e-4 and float(vel0[:, 2:4].norm(dim=1).max()) <= 8 + 1e-4
    return pos0, vel0, rep


# ---------------------------------------------------------------- bouncing ----
def bounce_replay(pos0, vel0, R):
    """float64 replay of the 2-D bouncing cell on all four columns, substep by
    substep.  Per sequence: margin (the closest any wall comparison came to
    its threshold, px), up / low (hits of the upper / lower wall per column,
    [B, 4]) and ac (substeps in which the upper reflection landed beyond the
    lower wall, flags a and c together, per column [B, 4])."""
    h = cell_dt().double() / 5
    p, v = pos0.double().clone(), vel0.double().clone()
    B = p.shape[0]
    margin = torch.full((B,), float("inf"), dtype=torch.float64)
    up, low, ac = (torch.zeros(B, 4, dtype=torch.long) for _ in range(3))
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
            ac += a & c
        ends_p.append(p)
        ends_v.append(v)
    return {"margin": margin, "up": up, "low": low, "ac": ac, "pos": torch.stack(ends_p), "vel": torch.stack(ends_v)}


def _bounce_pick(pos0, vel0, B, R, what, also=None):
    ok = bounce_replay(pos0, vel0, R)["margin"] >= BOUNCE_MARGIN
    if also is not None:
        ok = ok & also(bounce_replay(pos0, vel0, R))
    keep = _keep_first(ok, B, what)
    pos0, vel0 = pos0[keep].contiguous(), vel0[keep].contiguous()
    rep = bounce_replay(pos0, vel0, R)
    op, ov = cell_steps(BOUNCE2D, pos0, vel0, R, {})
    assert torch.equal(rep["pos"], op) and torch.equal(rep["vel"], ov), what
    assert bool((rep["margin"] >= BOUNCE_MARGIN).all()), what
    return pos0, vel0, rep


def _bounce_candidates(n, g):
    return 4 + 24 * torch.rand(n, 4, generator=g), 80 * torch.rand(n, 4, generator=g) - 40


@functools.lru_cache(maxsize=None)
def bouncing_inputs(B, R, seed=0, zero_vel=False):
    """(pos0, vel0 [B, 4] fp32, replay): rollout_cases.bouncing_inputs' recipe
    on all four columns, pos0 ~ U[4, 28], vel0 ~ U[-40, 40]."""
    g = torch.Generator().manual_seed(1000 * R + B + seed)
    pos0, vel0 = _bounce_candidates(CANDIDATES * B, g)
    if zero_vel:
        vel0 = torch.zeros_like(vel0)
    return _bounce_pick(pos0, vel0, B, R, f"bouncing 2-D B={B} R={R}")


@functools.lru_cache(maxsize=None)
def bouncing_overshoot_inputs(B=8, R=2, seed=0):
    """|vel0| in [950, 1200] on column 2 (object 1's x): one substep carries it
    so far past the far wall that its reflection lies beyond the near wall
    (h |v| >= 57 px on a 28 px court): flags a and c together."""
    g = torch.Generator().manual_seed(77 + seed)
    n = CANDIDATES * B
    pos0, vel0 = _bounce_candidates(n, g)
    mag = 950 + 250 * torch.rand(n, generator=g)
    vel0[:, 2] = torch.where(torch.arange(n) % 2 == 0, mag, -mag)
    pos0, vel0, rep = _bounce_pick(pos0, vel0, B, R, "bouncing 2-D overshoot", also=lambda r: r["ac"][:, 2] >= 1)
    assert bool((vel0[:, 2].abs() > 480).all()) and bool((rep["ac"][:, 2] >= 1).all())
    return pos0, vel0, rep
