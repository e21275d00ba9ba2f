"""The streaming device renderer on the GPU: paig_synth_draw against its host
twin, paig_synth_compact against np.flatnonzero, paig_synth_raster_ex's skipped
rows, StreamingDeviceIterator against the pieces it is made of (draw ->
integrate -> compact -> raster, run here round by round), its shortfall rule,
and training steps fed by it (eager and graph replay, byte targets bound)
against the same steps on the recorded batches.

Bounds.  Uniforms: bit-equal (integer arithmetic and exact float conversions).
p0 / v0: 1e-12 px absolute -- the values are <= 64 and differ from the twin's
only through sin / cos / sqrt, a few ulp (<= ~1e-14 px); everything else is the
same IEEE operation on both sides.  Bytes: equal."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from paig_reproduction_amd.nn.datasets import synth_device as S
from paig_reproduction_amd.nn.datasets.iterators import StreamingDeviceIterator

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- paig_synth_draw -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twin(task):
    return S.initial_conditions_philox(task, 9, 3, 5, 200, return_uniforms=True)


# phys 0 / half / the 64 x 64 scaling / phys 1 / phys 2
@pytest.mark.parametrize("task", ["spring_color", "spring_color_half", "mnist_spring_color", "bouncing_balls",
                                  "3bp_color"])
def test_draw_matches_twin(task):
    pt, vt, ut = _twin(task)
    K = pt.shape[1]
    worst = 0.0
    for m in (1, 63, 64, 65, 200):
        # guard rows after the m candidates: the kernel writes exactly m
        p = torch.full((m + 3, K, 2), -7.0, dtype=torch.float64, device=DEV)
        v, u = torch.full_like(p, -7.0), torch.full((m + 3, S.DRAW_U), -7.0, dtype=torch.float64, device=DEV)
        S.draw_device(task, 9, 3, 5, m, device=DEV, p0=p[:m], v0=v[:m], uniforms=u[:m])
        p, v, u = p.cpu().numpy(), v.cpu().numpy(), u.cpu().numpy()
        assert (p[m:] == -7).all() and (v[m:] == -7).all() and (u[m:] == -7).all()
        assert np.array_equal(u[:m], ut[:m]), f"m={m}: uniforms differ"
        d = max(np.abs(p[:m] - pt[:m]).max(), np.abs(v[:m] - vt[:m]).max())
        worst = max(worst, float(d))
        assert d <= 1e-12, (m, d)
    print(f"\n{task}: worst |device - twin| over p0, v0 = {worst:.3e} px")
    # without the debug output: the same states
    p2, v2 = S.draw_device(task, 9, 3, 5, 65, device=DEV)
    p3 = torch.empty_like(p2)
    v3 = torch.empty_like(v2)
    S.draw_device(task, 9, 3, 5, 65, p0=p3, v0=v3, uniforms=torch.empty((65, S.DRAW_U), dtype=torch.float64, device=DEV))
    assert torch.equal(p2, p3) and torch.equal(v2, v3)
    # another round / stream id / seed: other candidates
    for key in ((9, 3, 6), (9, 4, 5), (10, 3, 5)):
        assert not torch.equal(S.draw_device(task, *key, 65, device=DEV)[0], p2)


def test_background_matches_twin():
    out = torch.full((3, 64, 64), -1.0, device=DEV)
    S.background_device(4, 1, 7, out[:2])
    got = out.cpu().numpy()
    assert np.array_equal(got[:2], S.background_philox(4, 1, 7, 2, 64)) and (got[2] == -1).all()


# ---- paig_synth_compact --------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 4096 + 37])
def test_compact_matches_flatnonzero(m):
    rng = np.random.default_rng(m)
    cases = {"none": np.zeros(m, np.int32), "all": np.ones(m, np.int32),
             "random": (rng.random(m) < 0.4).astype(np.int32),
             "values": ((rng.random(m) < 0.5) * rng.integers(-5, 6, m)).astype(np.int32)}   # any nonzero is set
    for name, flags in cases.items():
        want = np.flatnonzero(flags)
        a = want.size
        valid = torch.from_numpy(flags).to(DEV)
        for n in sorted({0, max(a - 1, 0), a, a + 1, a + 70, 1}):
            for sentinel in (None, 777):
                # rows is a view of a longer buffer: what lies past n is not the kernel's
                buf = torch.full((n + 5,), 777 if sentinel else 0, dtype=torch.int64, device=DEV)
                count = torch.full((2,), -3, dtype=torch.int32, device=DEV)
                totals = torch.tensor([10, 20, 30], dtype=torch.int64, device=DEV)
                S.compact_device(valid, n, rows=buf[:n], count=count, totals=totals)
                got, c, t = buf.cpu().numpy(), count.cpu().numpy(), totals.cpu().numpy()
                k = min(a, n)
                where = (name, m, n, sentinel)
                assert np.array_equal(got[:k], want[:k]), where
                assert (got[k:n] == -1).all(), where
                assert (got[n:] == (777 if sentinel else 0)).all(), where
                assert c.tolist() == [k, a], where
                assert t.tolist() == [11, 20 + k, 30 + n - k], where
        # fresh outputs, no totals
        rows, count = S.compact_device(valid, 4)
        assert rows.cpu().tolist() == (want[:4].tolist() + [-1] * 4)[:4] and count.cpu().tolist() == [min(a, 4), a]


# ---- paig_synth_raster_ex ------------------------------------------------------------------------
@pytest.mark.parametrize("size,K,radius,with_bg", [(32, 2, 2.0, False), (32, 3, 2.0, False), (36, 3, 2.0, False), (64, 2, 6.0, True)])
def test_raster_skips_negative_rows(size, K, radius, with_bg):
    m, T = 7, 3
    g = torch.Generator().manual_seed(size)
    pos = (radius + (size - 2 * radius) * torch.rand((m, T, K, 2), generator=g, dtype=torch.float64)).to(DEV)
    rows = [-1, 2, 6, -1, 0, m, 4, -1]          # skipped: first, interior, out of range (>= m), last
    n = len(rows)
    keep = [i for i, r in enumerate(rows) if 0 <= r < m]
    bg = (torch.rand((n, size, size), generator=g) - 0.2).clamp_(0, 1).to(DEV) if with_bg else None
    out = torch.full((n, T, size, size, 3), 0xA5, dtype=torch.uint8, device=DEV)
    S.rasterize_rows_device(pos, size, radius, torch.tensor(rows, dtype=torch.int64, device=DEV), out, bg=bg)
    want = S.rasterize_device(pos, size, radius, rows=[rows[i] for i in keep],
                              bg=None if bg is None else bg[keep].contiguous())
    for j, i in enumerate(keep):
        assert torch.equal(out[i], want[j]), (i, rows[i])
        assert int(out[i].max()) > 0
    for i in set(range(n)) - set(keep):
        assert bool((out[i] == 0xA5).all()), (i, rows[i])


# ---- the iterator against its pieces -------------------------------------------------------------
def _round(task, seed, rank, rnd, cand, T, n):
    """One refill as the test composes it: (uint8 [n, T, H, W, 3] over zeros, count)."""
    q = S.task_params(task)
    p0, v0 = S.draw_device(task, seed, rank, rnd, cand, device=DEV)
    pos, valid = S.integrate_device(task, p0, v0, T)
    rows, count = S.compact_device(valid, n)
    out = torch.zeros((n, T, q["size"], q["size"], 3), dtype=torch.uint8, device=DEV)
    bg = None
    if task == "mnist_spring_color":
        bg = S.background_device(seed, rank, rnd, torch.empty((n, q["size"], q["size"]), device=DEV))
    S.rasterize_rows_device(pos, q["size"], q["draw"], rows, out, bg=bg)
    return out, count.cpu().tolist()


def _bytes(x):
    """A gathered float batch [B, T, 3, H, W] (Q5: the NHWC bytes / 255) -> uint8 [B, T, H, W, 3]."""
    b = torch.round(x * 255.0)
    assert float((x * 255.0 - b).abs().max()) < 1e-3
    return b.to(torch.uint8).reshape(x.shape[0], x.shape[1], x.shape[3], x.shape[4], 3)


def _batches(it, B, k):
    return [_bytes(it.next_batch(B)[0]) for _ in range(k)]


CASES = {"bouncing_balls": (12, 8, 64), "spring_color": (12, 8, 64), "3bp_color": (20, 4, None),
         "mnist_spring_color": (12, 4, None)}


@pytest.mark.parametrize("task", list(CASES))
def test_iterator_equals_its_pieces(task):
    T, B, cand = CASES[task]
    seed = 0
    it = StreamingDeviceIterator(task, T, B, DEV, epoch_size=3 * B + 1, seed=seed, candidates=cand)
    assert it.X.shape[0] == 2 * B and it.num_examples == 3 * B + 1
    assert it.candidates == (cand or S.default_candidates(task, T, B))
    got = _batches(it, B, 6)
    assert it.epochs_completed == 2
    for r in range(6):
        want, count = _round(task, seed, 0, r, it.candidates, T, B)
        assert count[0] == B <= count[1], (r, count)      # nothing below is vacuous
        assert torch.equal(got[r], want), f"batch {r}"
        assert all(int(want[i].max()) > 0 for i in range(B))
    for r in range(5):
        assert not torch.equal(got[r], got[r + 1])
    st = it.stats()
    assert st["refills"] == 5 and st["shortfall_slots"] == 0 and st["accepted_per_refill"] == B
    assert st["construction_rounds"] == 2
    # the same seed: the same stream; another rank: another
    again = StreamingDeviceIterator(task, T, B, DEV, epoch_size=3 * B + 1, seed=seed, candidates=cand)
    other = StreamingDeviceIterator(task, T, B, DEV, epoch_size=3 * B + 1, seed=seed, candidates=cand, rank=1, world=2)
    g2, g3 = _batches(again, B, 4), _batches(other, B, 4)
    assert other.epochs_completed == 4                    # 3 B + 1 sequences over 2 ranks: 1 batch an epoch
    for r in range(4):
        assert torch.equal(g2[r], got[r]) and not torch.equal(g3[r], got[r])
    from paig_reproduction_amd._lib import PaigError
    with pytest.raises(PaigError):
        it.next_batch(B + 1)
    with pytest.raises(PaigError):
        it.next_batch(B - 1)


def test_iterator_depth3_and_side_stream():
    """Three halves, and steps on a stream that is not the default one."""
    task, T, B = "bouncing_balls", 12, 8
    it = StreamingDeviceIterator(task, T, B, DEV, epoch_size=100, seed=2, candidates=64, depth=3)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got = _batches(it, B, 7)
    torch.cuda.synchronize()
    for r in range(7):
        assert torch.equal(got[r], _round(task, 2, 0, r, 64, T, B)[0]), r


def test_shortfall_keeps_previous_sequences():
    task, T, B, cand, seed = "spring_color", 50, 8, 64, 0
    it = StreamingDeviceIterator(task, T, B, DEV, epoch_size=64, seed=seed, candidates=cand)
    assert it.construction_rounds > 2                    # ~2.5 of 64 accepted a round: top-ups ran
    got = _batches(it, B, 6)
    for r in (0, 1):                                     # construction wrote every slot
        assert all(int(got[r][i].max()) > 0 for i in range(B))
    short = 0
    for r in range(2, 6):
        want, (c, acc) = _round(task, seed, 0, r, cand, T, B)
        assert c == acc < B, (r, c, acc)                 # a shortfall in every refill compared here
        assert torch.equal(got[r][:c], want[:c]), r
        assert torch.equal(got[r][c:], got[r - 2][c:]), r     # the previous batch of this half, byte for byte
        short += B - c
    # the 6 calls issued refills of batches 2 .. 6
    short += B - _round(task, seed, 0, 6, cand, T, B)[1][0]
    st = it.stats()
    assert st["refills"] == 5 and st["shortfall_slots"] == short > 0
    assert st["accepted_per_refill"] == (5 * B - short) / 5


# ---- training steps fed by the stream ------------------------------------------------------------
INS, PRED, SEQ, TB, STEPS = 4, 6, 12, 8, 6     # the step split of the spring_s12 fixture


def _train(feed, graph, bind_it=None):
    """STEPS steps (2 eager, then the capture and replays when ``graph``):
    per-step losses and the final flat parameter buffers."""
    from paig_reproduction_amd.graph_step import GraphStep
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    torch.manual_seed(0)
    m = PhysicsNet("spring_color", 100, 1, "spring_ode_cell", SEQ, INS, PRED, 3.0, False, True, 32 * 32, "conv_encoder",
                   "conv_st_decoder", device=DEV).to(DEV)
    m.build_optimizer(1e-3, "rmsprop", True)
    xbuf = torch.full((TB, SEQ, 3, 32, 32), float("nan"), device=DEV)
    gs = GraphStep(m, xbuf, 1, graph=graph)
    if bind_it is not None:
        gs.eng.byte_targets = bind_it.bind_targets(xbuf, INS + PRED)
    losses = []
    for s in range(STEPS):
        if graph and s == 2:
            gs.capture()
        feed(s, xbuf)
        losses.append((gs() if graph and s >= 2 else gs.eager()).detach().clone())
    gs.finish()
    torch.cuda.synchronize()
    return torch.stack(losses), m._flat.p32.clone(), m._flat.p64.clone()


def _stream_it():
    return StreamingDeviceIterator("spring_color", SEQ, TB, DEV, epoch_size=1000, seed=3, candidates=64)


@functools.lru_cache(maxsize=None)
def _recorded():
    """The stream's first STEPS batches, resident: float32 [STEPS, B, T, 3, 32, 32]."""
    it = _stream_it()
    rec = torch.stack([it.next_batch(TB)[0].clone() for _ in range(STEPS)])
    assert it.stats()["shortfall_slots"] == 0
    for s in range(STEPS - 1):
        assert not torch.equal(rec[s], rec[s + 1])
    return rec


@functools.lru_cache(maxsize=None)
def _reference(graph):
    rec = _recorded()
    return _train(lambda s, xbuf: xbuf.copy_(rec[s]), graph)


@pytest.mark.parametrize("graph", [False, True])
def test_training_on_the_stream_bit_identical(graph):
    it = _stream_it()
    got = _train(lambda s, xbuf: it.next_batch(TB, out=xbuf), graph, bind_it=it)
    want = _reference(graph)
    assert bool(torch.isfinite(want[0]).all())
    assert torch.equal(got[0], want[0]), (got[0].tolist(), want[0].tolist())
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert not torch.equal(want[0][1:], want[0][:-1])     # the losses move: the steps saw different batches


# ---- the runner ----------------------------------------------------------------------------------
def test_runner_streams_and_touches_no_data_dir(tmp_path):
    import logging
    sys.path.insert(0, os.path.join(REPO, "runners"))
    import torch_run_physics as R
    lg = logging.getLogger("torch")
    handlers, level = list(lg.handlers), lg.level
    save, data = str(tmp_path / "run"), str(tmp_path / "data")
    try:
        net = R.main(["--task", "spring_color", "--color", "--autoencoder_loss", "3.0", "--epochs", "2",
                      "--batch_size", "10", "--save_dir", save, "--save_every_n_epochs", "1", "--print_interval", "1", "--data_dir", data,
                      "--synthetic", "40", "--synthetic_stream", "1", "--seed", "0"])
    finally:
        for h in list(lg.handlers):
            if h not in handlers:
                lg.removeHandler(h)
        lg.setLevel(level)
    assert not os.path.exists(data)
    log = open(os.path.join(save, "log.txt")).read()
    lines = [ln for ln in log.splitlines() if "stream - epoch=" in ln]
    assert len(lines) == 2 and "refills=7 " in lines[1] and "shortfall_slots=0" in lines[1], lines
    assert net.output.shape[1] == 30 - 4 and bool(torch.isfinite(net.output).all())
    with pytest.raises(SystemExit):
        R.main(["--task", "spring_color", "--color", "--synthetic_stream", "1"])
    with pytest.raises(SystemExit):
        R.main(["--task", "spring_color", "--color", "--synthetic_stream", "1", "--synthetic", "40", "--device_data", "0"])
