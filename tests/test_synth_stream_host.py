"""The host side of the streaming device renderer, no GPU: the Philox4x32-10
twin of paig_synth_draw (synth_device.initial_conditions_philox) and the
schedule of StreamingDeviceIterator (iterators.StreamPlan)."""
import numpy as np
import pytest

from paig_reproduction_amd.nn.datasets import synth_device as S
from paig_reproduction_amd.nn.datasets.iterators import StreamPlan

# Random123's known-answer vectors for philox4x32 with 10 rounds (kat_vectors):
# (counter, key, expected)
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
TASKS = ("spring_color", "spring_color_half", "mnist_spring_color", "bouncing_balls", "3bp_color")


def _philox_scalar(ctr, key):
    """The published round function, one block, in Python integers."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return tuple(c)


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert _philox_scalar(ctr, key) == want
        got = S.philox4x32_10(np.array(ctr), np.array(key))
        assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want
    # vectorised over counters and keys alike
    got = S.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
    assert [tuple(int(x) for x in r) for r in got] == [k[2] for k in KAT]
    rng = np.random.default_rng(0)
    ctr, key = rng.integers(0, 2 ** 32, (50, 4)), rng.integers(0, 2 ** 32, (50, 2))
    got = S.philox4x32_10(ctr, key)
    for c, k, g in zip(ctr.tolist(), key.tolist(), got.tolist()):
        assert _philox_scalar(c, k) == tuple(g)


def test_double_construction_exact():
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.integers(0, 2 ** 32, 200), [0, 0xffffffff, 0, 0xffffffff]]).astype(np.uint32)
    b = np.concatenate([rng.integers(0, 2 ** 32, 200), [0, 0xffffffff, 0xffffffff, 0]]).astype(np.uint32)
    u = S.u53(a, b)
    for x, y, v in zip(a.tolist(), b.tolist(), u.tolist()):
        assert Fraction(v) == Fraction((x >> 5) * 2 ** 26 + (y >> 6), 2 ** 53)
    assert u.min() == 0.0 and u.max() == 1.0 - 2.0 ** -53
    # the uniforms of a call are those words, slot by slot
    un = S.philox_uniforms(3, 1, 2, 5)
    w = np.array([[_philox_scalar((i, 0, 2, s), (3, 1)) for s in range(4)] for i in range(5)], dtype=np.uint32)
    assert np.array_equal(un[:, 0::2], S.u53(w[..., 0], w[..., 1]))
    assert np.array_equal(un[:, 1::2], S.u53(w[..., 2], w[..., 3]))


@pytest.mark.parametrize("task", TASKS)
def test_draws_inside_support(task):
    q = S.task_params(task)
    m = 4000
    p, v, u = S.initial_conditions_philox(task, 11, 2, 7, m, return_uniforms=True)
    assert p.shape == v.shape == (m, q["K"], 2) and p.dtype == v.dtype == np.float64
    assert u.shape == (m, S.DRAW_U) and (u >= 0).all() and (u < 1).all()
    size, rb = q["size"], q["bound"]
    eps = 1e-9
    if q["phys"] == "spring":
        equil, vmax = q["c1"], q["vmax"]
        cm = p.mean(1)
        lo, hi = rb + equil, size - (rb + equil)
        assert (cm >= lo - eps).all() and (cm[:, 1] <= hi + eps).all()
        assert (cm[:, 0] <= (size / 2 if q["half"] else hi) + eps).all()
        if q["half"]:
            assert cm[:, 0].max() > 0.9 * size / 2   # and not a narrower range
        d = np.linalg.norm(p[:, 0] - p[:, 1], axis=1) / 2
        assert (d >= 0.5 * equil - eps).all() and (d <= 1.5 * equil + eps).all()
        assert (np.linalg.norm(v, axis=2) <= vmax + eps).all()
    elif q["phys"] == "bounce":
        assert (p >= rb).all() and (p <= size - rb).all()
        sp = np.linalg.norm(v, axis=2)
        assert (sp >= 0.5 * q["vmax"] - eps).all() and (sp <= q["vmax"] + eps).all()
    else:
        c = size / 2
        r = np.linalg.norm(p - c, axis=2)
        assert (r >= 4 - eps).all() and (r <= 8 + eps).all()
        assert np.abs(r - r[:, :1]).max() < 1e-9                         # one orbit radius per candidate
        assert np.abs(p.mean(1) - c).max() < 1e-9                        # 120 degrees apart
        assert np.abs(np.linalg.norm(v, axis=2) - np.sqrt(q["c0"] / r) * 0.35).max() < 1e-9
        assert np.abs(((p - c) * v).sum(2)).max() < 1e-9                 # tangential
    # distributions, loosely: the uniforms fill [0, 1)
    used = 2 if q["phys"] == "gravity" else S.DRAW_U
    assert np.abs(u[:, :used].mean(0) - 0.5).max() < 0.03


@pytest.mark.parametrize("task", TASKS)
def test_prefix_and_key_separation(task):
    a, b = 37, 200
    pa, va = S.initial_conditions_philox(task, 5, 0, 3, a)
    pb, vb = S.initial_conditions_philox(task, 5, 0, 3, b)
    assert np.array_equal(pa, pb[:a]) and np.array_equal(va, vb[:a])
    for other in ((6, 0, 3), (5, 1, 3), (5, 0, 4)):   # seed, stream (rank), round
        po, _ = S.initial_conditions_philox(task, *other, a)
        assert not np.array_equal(po, pa)
    with pytest.raises(ValueError):
        S.initial_conditions_philox(task, 2 ** 32, 0, 0, 4)


def test_acceptance_rates_and_default_candidates():
    # the rates the default candidate count rests on (4096 numpy-drawn candidates gave
    # ~40 % / ~3.9 % / ~68 % / 100 % / 100 %)
    want = {("spring_color", 12): 0.40, ("spring_color", 50): 0.039, ("mnist_spring_color", 12): 0.68,
            ("3bp_color", 20): 1.0, ("bouncing_balls", 12): 1.0}
    for (task, T), r in want.items():
        got = S.acceptance_rate(task, T)
        assert abs(got - r) <= 0.15 * r + 1e-12, (task, T, got)
        for B in (8, 100):
            m = S.default_candidates(task, T, B)
            assert m % 64 == 0 and m * got >= 1.5 * B


def test_background_twin():
    bg = S.background_philox(1, 0, 4, 3, 64)
    assert bg.shape == (3, 64, 64) and bg.dtype == np.float32
    assert bg.min() == 0.0 and bg.max() <= 0.8
    assert abs(float((bg == 0).mean()) - 0.2) < 0.02
    assert np.array_equal(bg[:2], S.background_philox(1, 0, 4, 2, 64))


# ---- the planner -------------------------------------------------------------------------------
def _simulate(depth, calls, B=4):
    """Issue order of every operation on the two streams: a list of
    (stream, op) with the plan's waits resolved to positions."""
    plan = StreamPlan(depth, B, 100 * B)
    log = [("refill", op) for op in plan.start()]
    for _ in range(calls):
        for op in plan.next(B):
            log.append(("refill" if op[0] == "refill" else "compute", op))
    return log


@pytest.mark.parametrize("depth", [2, 3])
def test_plan_orders_refills_and_gathers(depth):
    log = _simulate(depth, 7)
    ops = [op for _, op in log]
    at = {op: i for i, op in enumerate(ops)}
    gathers = [op for op in ops if op[0] == "gather"]
    assert [g[2] for g in gathers] == list(range(7)) and all(g[1] == g[2] % depth for g in gathers)
    # what each half holds as the operations are issued
    holds = {}
    for op in ops:
        if op[0] == "fill":
            holds[op[1]] = op[2]
        elif op[0] == "refill":
            _, half, batch, wait = op
            assert half == batch % depth
            # ordered after the event that follows the step reading the half's previous batch
            prev = holds[half]
            assert wait == ("done", prev) and prev == batch - depth
            rec = at[("record", "done", prev)]
            assert at[("gather", half, prev)] < rec < at[op]
            # and that event is recorded before any later step's gather: it closes step `prev` exactly
            assert rec < at[("gather", (prev + 1) % depth, prev + 1)]
            holds[half] = batch
        elif op[0] == "wait":
            _, kind, half, k = op
            assert kind == "filled" and holds[half] == k, (op, holds)   # its refill (or fill) was issued before
            assert at[op] < at[("gather", half, k)]
        elif op[0] == "gather":
            assert holds[op[1]] == op[2]
            assert ("wait", "filled", op[1], op[2]) in at
    # every batch past the construction is refilled exactly once, one call ahead of need for depth 2
    refills = [op for op in ops if op[0] == "refill"]
    assert [r[2] for r in refills] == list(range(depth, depth + 6))
    # the refill of a call is issued before that call's gather (it runs under that step)
    for r in refills:
        k = r[3][1] + 1
        assert at[r] < at[("gather", k % depth, k)]


def test_plan_batch_size_and_epochs():
    B = 4
    plan = StreamPlan(2, B, 3 * B + 1)
    with pytest.raises(ValueError):
        plan.next(B + 1)
    with pytest.raises(ValueError):
        plan.next(B - 1)
    assert plan.k == 0
    for world, per_epoch in ((1, 3), (2, 1)):
        plan = StreamPlan(2, B, 3 * B + 1, world)
        seen = []
        for _ in range(7):
            plan.next(B)
            seen.append(plan.epochs_completed)
        assert seen == [(i + 1) // per_epoch for i in range(7)], (world, seen)
        plan.reset_epoch()
        assert plan.epochs_completed == 0
    with pytest.raises(ValueError):
        StreamPlan(2, B, B - 1)
    with pytest.raises(ValueError):
        StreamPlan(2, B, 2 * B - 1, world=2)
