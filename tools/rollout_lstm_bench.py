#!/usr/bin/env python3
"""Time of the black-box rollout cell beside the physics cells it replaces:
paig_rollout_lstm_fwd / _bwd (H = 100) and paig_rollout_fwd / _bwd of the 1-D
and 2-D spring and bouncing cells, at spring_color's headline shape (B = 100,
R = 46) and at bouncing's largest one (B = 1024, R = 96), in one process.

Device events around each call, WARMUP untimed calls, the median of RUNS timed
ones, each waited for under its own time limit (tools/rollout2d_bench.py's
timing loop and inputs).  The LSTM backward is the BPTT launch plus the three
weight-gradient GEMMs and three column sums.

    python tools/rollout_lstm_bench.py [--out profiles/rollout_lstm.json]

Prints one JSON line (and writes it to --out).  Needs the GPU; there is no
CPU fallback.
"""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import rollout2d_bench as R2   # noqa: E402

SHAPES = ((100, 46, (0, 3)), (1024, 96, (1, 4)))   # (B, R, physics kinds timed beside the LSTM)
D, H, HALF = 4, 100, 16.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--limit", type=float, default=20.0, help="seconds allowed to each timed call")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_lstm_bench: needs the GPU (no CPU fallback)")
    from paig_reproduction_amd._lib import lib, ptr, stream_handle
    from paig_reproduction_amd.nn.network.cells import lstm_ode_cell
    L = lib()
    dev = torch.device("cuda:0")
    st = stream_handle(dev)
    dt = torch.tensor(0.3, device=dev)
    k = torch.tensor(math.log(2.0), dtype=torch.float64, device=dev)
    eq = torch.tensor(math.log(3.0), dtype=torch.float64, device=dev)
    torch.manual_seed(0)
    cell = lstm_ode_cell(D, D, H, HALF).to(dev)
    W = [p.detach() for p in cell.weights()]
    rows = []
    for B, R, kinds in SHAPES:
        g = torch.Generator().manual_seed(B + R)
        dpos_roll = torch.randn(B, R, D, generator=g).to(dev)
        dpvs = torch.randn(B, R + 1, 2 * D, generator=g).to(dev)
        pvs = torch.empty(B, R + 1, 2 * D, device=dev)
        dpos0, dvel0 = torch.empty(B, D, device=dev), torch.empty(D // 2, B, 2, device=dev)
        # ---- the LSTM cell
        pos0, vk = R2.inputs(1, B, dev)
        vk = vk * 0.1
        nws = L.paig_rollout_lstm_workspace(B, D, H, R)
        ws = torch.empty(nws // 4, device=dev)
        grads = [torch.empty_like(w) for w in W]

        def lfwd(ws=ws, nws=nws):
            L.paig_rollout_lstm_fwd(ptr(pos0), D, ptr(vk), *[ptr(w) for w in W], HALF, ptr(pvs), ptr(ws), nws, B, D, H,
                                    R, st)

        def lfwd_eval():
            L.paig_rollout_lstm_fwd(ptr(pos0), D, ptr(vk), *[ptr(w) for w in W], HALF, ptr(pvs), None, 0, B, D, H, R, st)

        def lbwd():
            L.paig_rollout_lstm_bwd(ptr(dpos_roll), ptr(dpvs), ptr(W[0]), ptr(W[1]), ptr(W[4]), HALF, ptr(dpos0),
                                    ptr(dvel0), *[ptr(t) for t in grads], 0, ptr(ws), nws, B, D, H, R, st)

        what = f"lstm B={B} R={R} H={H}"
        f_med, f_min = R2.timed(lfwd, what + " fwd", a.warmup, a.runs, a.limit)
        e_med, e_min = R2.timed(lfwd_eval, what + " fwd (no workspace)", a.warmup, a.runs, a.limit)
        b_med, b_min = R2.timed(lbwd, what + " bwd", a.warmup, a.runs, a.limit)
        if not all(bool(torch.isfinite(t).all()) for t in [pvs, dpos0] + grads):
            raise SystemExit(f"rollout_lstm_bench: {what}: non-finite result")
        rows.append({"cell": "lstm", "B": B, "R": R, "H": H, "fwd_us": f_med, "fwd_us_min": f_min,
                     "fwd_eval_us": e_med, "fwd_eval_us_min": e_min, "bwd_us": b_med, "bwd_us_min": b_min,
                     "workspace_bytes": int(nws)})
        # ---- the physics cells at the same shape
        for kind in kinds:
            name = R2.KINDS[kind]
            pos0k, vkk = R2.inputs(kind, B, dev)
            p0, p1 = (k, eq) if kind in (0, 3) else (None, None)
            part = torch.empty(2 * L.paig_rollout_bwd_blocks(B), dtype=torch.float64, device=dev)
            gq = torch.zeros(2, dtype=torch.float64, device=dev)

            def fwd():
                L.paig_rollout_fwd(kind, ptr(pos0k), D, ptr(vkk), ptr(dt), ptr(p0), ptr(p1), ptr(pvs), B, D, R, st)

            def bwd():
                L.paig_rollout_bwd(kind, ptr(pvs), ptr(dpos_roll), ptr(dpvs), ptr(dt), ptr(p0), ptr(p1), ptr(dpos0),
                                   ptr(dvel0), ptr(part), ptr(gq), ptr(gq) + 8, 0, B, D, R, st)

            what = f"{name} B={B} R={R}"
            f_med, f_min = R2.timed(fwd, what + " fwd", a.warmup, a.runs, a.limit)
            b_med, b_min = R2.timed(bwd, what + " bwd", a.warmup, a.runs, a.limit)
            rows.append({"cell": name, "kind": kind, "B": B, "R": R, "fwd_us": f_med, "fwd_us_min": f_min,
                         "bwd_us": b_med, "bwd_us_min": b_min})
    out = {"tool": "tools/rollout_lstm_bench.py", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "runs": a.runs, "statistic": "median of device-event times per call (us); min beside it",
           "note": "lstm bwd = the BPTT launch + 3 fp32 GEMMs (dW_ih, dW_hh, dW_p) + 3 column sums; physics bwd = "
                   "the adjoint launch + the parameter finalisation launch",
           "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
