"""Times the device renderer (csrc/synth.hip) against the host renderer.

Per shape -- spring_color n = 100, T = 50 (one benchmark batch) and
bouncing_balls n = 1024, T = 100 -- the integrator (one round of `chunk`
candidates) and the rasteriser (n accepted sequences) are timed separately
with HIP events after warm-up (median of --runs), the whole
render_sequences_device call (host draws, upload, rounds and their flag reads
included) with a host clock around a synchronise, and synth.render_sequences
for 8 sequences on the host.  Writes one JSON file.

    PYTHONPATH=. python tools/render_bench.py --out profiles/synth_device.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from paig_reproduction_amd.nn.datasets import synth  # noqa: E402
from paig_reproduction_amd.nn.datasets import synth_device as SD  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, MI355X
STEP_MS = 1.031        # the training step one benchmark batch feeds (BENCH_r06.json)
SHAPES = (("spring_color", 100, 50), ("bouncing_balls", 1024, 100))


def event_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def bench_shape(task, n, T, chunk, warmup, runs, dev):
    q = SD.task_params(task)
    size = q["size"]
    rng = np.random.default_rng(0)
    p0, v0 = SD.initial_conditions(task, rng, chunk)
    p0d, v0d = torch.from_numpy(p0).to(dev), torch.from_numpy(v0).to(dev)
    pos, valid = SD.integrate_device(task, p0d, v0d, T)
    ok = np.flatnonzero(valid.cpu().numpy())
    rows = np.resize(ok, n)                       # fewer than n accepted in one round: reuse them (timing only)
    rows_d = torch.from_numpy(rows).to(dev)
    out = torch.empty((n, T, size, size, 3), dtype=torch.uint8, device=dev)
    from paig_reproduction_amd._lib import lib, stream_handle
    st = stream_handle(dev)

    def raster():
        lib().paig_synth_raster(pos.data_ptr(), rows_d.data_ptr(), n, T, q["K"], size, float(q["draw"]), None,
                                out.data_ptr(), st)

    integ = event_ms(lambda: SD.integrate_device(task, p0d, v0d, T), warmup, runs)
    rast = event_ms(raster, warmup, runs)
    nbytes = out.numel()

    def whole():
        SD.render_sequences_device(task, n, T, seed=0, device=dev, chunk=chunk)
        torch.cuda.synchronize()

    walls = []
    for i in range(3 + 7):
        t0 = time.perf_counter()
        whole()
        if i >= 3:
            walls.append((time.perf_counter() - t0) * 1e3)
    # rounds the whole call needs
    rng2, got, rounds = np.random.default_rng(0), 0, 0
    while got < n:
        a, b = SD.initial_conditions(task, rng2, chunk)
        got += int(SD.integrate_device(task, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), T)[1].sum())
        rounds += 1
    t0 = time.perf_counter()
    synth.render_sequences(task, 8, T, seed=0)
    host_s = time.perf_counter() - t0
    wall = statistics.median(walls)
    return {
        "task": task, "n": n, "T": T, "size": size, "chunk": chunk,
        "integrate_ms": {"median": integ[0], "min": integ[1], "max": integ[2], "candidates": chunk},
        "raster_ms": {"median": rast[0], "min": rast[1], "max": rast[2]},
        "raster_bytes": nbytes,
        "raster_bytes_per_s": nbytes / (rast[0] * 1e-3),
        "raster_fraction_of_8TBps": nbytes / (rast[0] * 1e-3) / HBM_PEAK,
        "acceptance_rate": len(ok) / chunk,
        "rounds_for_n": rounds,
        "device_only_ms_for_n": rounds * integ[0] + rast[0],
        "render_sequences_device_wall_ms": {"median": wall, "min": min(walls), "max": max(walls)},
        "device_sequences_per_s": n / (wall * 1e-3),
        "host_render_sequences_8_s": host_s,
        "host_sequences_per_s": 8 / host_s,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "synth_device.json"))
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("render_bench times the GPU renderer: no HIP device found")
    assert args.runs >= 20
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "step_ms": STEP_MS,
           "shapes": [bench_shape(t, n, T, args.chunk, args.warmup, args.runs, dev) for t, n, T in SHAPES]}
    b = res["shapes"][0]
    res["benchmark_batch_fits_in_step"] = {
        "device_only": b["device_only_ms_for_n"] <= STEP_MS,
        "whole_call": b["render_sequences_device_wall_ms"]["median"] <= STEP_MS,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
