#!/usr/bin/env python3
"""Time of the rollout kernels per cell kind: paig_rollout_fwd and
paig_rollout_bwd for the reference's cells (0 spring, 1 bouncing) and the
opt-in 2-D cells (3 spring 2-D, 4 bouncing 2-D) at the headline shape
(B = 100, R = 46: spring_color, seq 50) and at the largest one in use
(B = 1024, R = 96), in one process.  The 1-D kinds are the baseline.

Device events around each call, WARMUP untimed calls, the median of RUNS
timed ones; every timed call is waited for under its own time limit (the tool
stops at the first call that exceeds it and starts nothing more).

    python tools/rollout2d_bench.py [--out profiles/rollout2d.json]

Prints one JSON line (and writes it to --out).  Needs the GPU; there is no
CPU fallback.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KINDS = {0: "spring", 1: "bouncing", 3: "spring2d", 4: "bouncing2d"}
SHAPES = ((100, 46), (1024, 96))
D = 4


def inputs(kind, B, dev):
    """States at which the cell's physics acts: spring ends 6-10 px apart
    around the centre with |v| <= 4, balls anywhere on the court at up to 40 px
    per time unit."""
    g = torch.Generator().manual_seed(17 * B + kind)
    if kind in (0, 3):
        c = 16 + 4 * (torch.rand(B, 2, generator=g) - 0.5)
        th = 2 * math.pi * torch.rand(B, generator=g)
        half = (3 + 2 * torch.rand(B, 1, generator=g)) * torch.stack([torch.cos(th), torch.sin(th)], -1)
        pos0 = torch.cat([c + half, c - half], 1)
        if kind == 0:   # split size 1: the spring joins columns 0 and 1
            pos0[:, 1] = pos0[:, 0] - (6 + 4 * torch.rand(B, generator=g))
        vel0 = 8 * (torch.rand(B, D, generator=g) - 0.5)
    else:
        pos0 = 4 + 24 * torch.rand(B, D, generator=g)
        vel0 = 80 * torch.rand(B, D, generator=g) - 40
    vk = vel0.view(B, D // 2, 2).permute(1, 0, 2).contiguous()
    return pos0.to(dev), vk.to(dev)


def wait(ev, limit, what):
    """Wait for the event, at most ``limit`` seconds."""
    t0 = time.monotonic()
    while not ev.query():
        if time.monotonic() - t0 > limit:
            raise SystemExit(f"rollout2d_bench: {what} did not finish within {limit:g} s; stopping")
        time.sleep(0.0005)


def timed(call, what, warmup, runs, limit):
    """Median (and min) device time of ``call`` in microseconds."""
    for _ in range(warmup):
        call()
    done = torch.cuda.Event()
    done.record()
    wait(done, limit, what + " (warm-up)")
    us = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        wait(b, limit, what)
        us.append(a.elapsed_time(b) * 1e3)
    us.sort()
    return round(us[len(us) // 2], 2), round(us[0], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--limit", type=float, default=20.0, help="seconds allowed to each timed call")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout2d_bench: needs the GPU (no CPU fallback)")
    from paig_reproduction_amd._lib import lib, ptr, stream_handle
    L = lib()
    dev = torch.device("cuda:0")
    st = stream_handle(dev)
    dt = torch.tensor(0.3, device=dev)
    k = torch.tensor(math.log(2.0), dtype=torch.float64, device=dev)
    eq = torch.tensor(math.log(3.0), dtype=torch.float64, device=dev)
    rows = []
    for B, R in SHAPES:
        g = torch.Generator().manual_seed(B + R)
        dpos_roll = torch.randn(B, R, D, generator=g).to(dev)
        dpvs = torch.randn(B, R + 1, 2 * D, generator=g).to(dev)
        for kind, name in KINDS.items():
            pos0, vk = inputs(kind, B, dev)
            p0, p1 = (k, eq) if kind in (0, 3) else (None, None)
            pvs = torch.empty(B, R + 1, 2 * D, device=dev)
            dpos0, dvel0 = torch.empty(B, D, device=dev), torch.empty(D // 2, B, 2, device=dev)
            part = torch.empty(2 * L.paig_rollout_bwd_blocks(B), dtype=torch.float64, device=dev)
            gq = torch.zeros(2, dtype=torch.float64, device=dev)

            def fwd():
                L.paig_rollout_fwd(kind, ptr(pos0), D, ptr(vk), ptr(dt), ptr(p0), ptr(p1), ptr(pvs), B, D, R, st)

            def bwd():
                L.paig_rollout_bwd(kind, ptr(pvs), ptr(dpos_roll), ptr(dpvs), ptr(dt), ptr(p0), ptr(p1), ptr(dpos0),
                                   ptr(dvel0), ptr(part), ptr(gq), ptr(gq) + 8, 0, B, D, R, st)

            what = f"{name} B={B} R={R}"
            f_med, f_min = timed(fwd, what + " fwd", a.warmup, a.runs, a.limit)
            b_med, b_min = timed(bwd, what + " bwd", a.warmup, a.runs, a.limit)
            if not (bool(torch.isfinite(pvs).all()) and bool(torch.isfinite(dpos0).all())):
                raise SystemExit(f"rollout2d_bench: {what}: non-finite result")
            rows.append({"kind": kind, "cell": name, "B": B, "R": R, "fwd_us": f_med, "fwd_us_min": f_min,
                         "bwd_us": b_med, "bwd_us_min": b_min})
    out = {"tool": "tools/rollout2d_bench.py", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "runs": a.runs, "statistic": "median of device-event times per call (us); min beside it",
           "note": "bwd = the adjoint launch + the parameter finalisation launch (kinds 0, 3); kind 0 at R <= 64 "
                   "is the scan adjoint, every other row the serial adjoint",
           "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
