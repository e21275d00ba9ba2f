#!/usr/bin/env python3
"""Time of the interaction-network rollout cell: paig_rollout_in_fwd / _bwd
(H = 100) at spring_color's headline shape (B = 100, R = 46) and at
bouncing's largest one (B = 1024, R = 96), beside the black-box LSTM cell at
the same shapes.

Device events around each call, WARMUP untimed calls, the median of RUNS timed
ones, each waited for under its own time limit (tools/rollout2d_bench.py's
timing loop and inputs; tools/rollout_lstm_bench.py's method).  The backward
is the BPTT launch plus the four weight-gradient GEMMs and four column sums.
The LSTM's figures are read from the JSON that tools/rollout_lstm_bench.py
wrote in the same session (--lstm); both cells' times, the measured ratio and
the ratio of their multiply-adds per sequence and step

    interaction:  K (K - 1) (8 H + H^2) + K ((4 + H) H + 4 H)
    LSTM:         4 H (2 D + H) + 2 D H

go into the result.

    python tools/rollout_lstm_bench.py --out /tmp/lstm.json
    python tools/rollout_in_bench.py --lstm /tmp/lstm.json [--out profiles/rollout_in.json]

Prints one JSON line (and writes it to --out).  Needs the GPU; there is no
CPU fallback.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import rollout2d_bench as R2   # noqa: E402

SHAPES = ((100, 46), (1024, 96))   # (B, R)
D, H, HALF = 4, 100, 16.0


def madds_in(D, H):
    K = D // 2
    return K * (K - 1) * (8 * H + H * H) + K * ((4 + H) * H + 4 * H)


def madds_lstm(D, H):
    return 4 * H * (2 * D + H) + 2 * D * H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--limit", type=float, default=20.0, help="seconds allowed to each timed call")
    ap.add_argument("--lstm", type=str, default="", help="tools/rollout_lstm_bench.py's JSON of the same session")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_in_bench: needs the GPU (no CPU fallback)")
    from paig_reproduction_amd._lib import lib, ptr, stream_handle
    from paig_reproduction_amd.nn.network.cells import interaction_ode_cell
    L = lib()
    dev = torch.device("cuda:0")
    st = stream_handle(dev)
    torch.manual_seed(0)
    cell = interaction_ode_cell(D, D, H, HALF).to(dev)
    W = [p.detach() for p in cell.weights()]
    lstm_rows = {}
    if a.lstm:
        with open(a.lstm) as f:
            lstm_rows = {(r["B"], r["R"]): r for r in json.load(f)["rows"] if r["cell"] == "lstm" and r["H"] == H}
    work = madds_in(D, H) / madds_lstm(D, H)
    rows = []
    for B, R in SHAPES:
        g = torch.Generator().manual_seed(B + R)
        dpos_roll = torch.randn(B, R, D, generator=g).to(dev)
        dpvs = torch.randn(B, R + 1, 2 * D, generator=g).to(dev)
        pvs = torch.empty(B, R + 1, 2 * D, device=dev)
        dpos0, dvel0 = torch.empty(B, D, device=dev), torch.empty(D // 2, B, 2, device=dev)
        pos0, vk = R2.inputs(1, B, dev)
        vk = vk * 0.1
        nws = L.paig_rollout_in_workspace(B, D, H, R)
        ws = torch.empty(nws // 4, device=dev)
        grads = [torch.empty_like(w) for w in W]

        def fwd():
            L.paig_rollout_in_fwd(ptr(pos0), D, ptr(vk), *[ptr(w) for w in W], HALF, ptr(pvs), ptr(ws), nws, B, D, H, R,
                                  st)

        def fwd_eval():
            L.paig_rollout_in_fwd(ptr(pos0), D, ptr(vk), *[ptr(w) for w in W], HALF, ptr(pvs), None, 0, B, D, H, R, st)

        def bwd():
            L.paig_rollout_in_bwd(ptr(dpos_roll), ptr(dpvs), ptr(W[0]), ptr(W[2]), ptr(W[4]), ptr(W[6]), HALF,
                                  ptr(dpos0), ptr(dvel0), *[ptr(t) for t in grads], 0, ptr(ws), nws, B, D, H, R, st)

        what = f"interaction B={B} R={R} H={H}"
        f_med, f_min = R2.timed(fwd, what + " fwd", a.warmup, a.runs, a.limit)
        e_med, e_min = R2.timed(fwd_eval, what + " fwd (no workspace)", a.warmup, a.runs, a.limit)
        b_med, b_min = R2.timed(bwd, what + " bwd", a.warmup, a.runs, a.limit)
        if not all(bool(torch.isfinite(t).all()) for t in [pvs, dpos0] + grads):
            raise SystemExit(f"rollout_in_bench: {what}: non-finite result")
        row = {"cell": "interaction", "B": B, "R": R, "D": D, "H": H, "fwd_us": f_med, "fwd_us_min": f_min,
               "fwd_eval_us": e_med, "fwd_eval_us_min": e_min, "bwd_us": b_med, "bwd_us_min": b_min,
               "workspace_bytes": int(nws)}
        ls = lstm_rows.get((B, R))
        if ls is not None:
            row["lstm"] = {k: ls[k] for k in ("fwd_us", "fwd_eval_us", "bwd_us")}
            row["ratio_measured"] = {"fwd": f_med / ls["fwd_us"], "bwd": b_med / ls["bwd_us"],
                                     "fwd_plus_bwd": (f_med + b_med) / (ls["fwd_us"] + ls["bwd_us"])}
        rows.append(row)
    out = {"tool": "tools/rollout_in_bench.py", "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "runs": a.runs, "statistic": "median of device-event times per call (us); min beside it",
           "note": "interaction bwd = the BPTT launch + 4 fp32 GEMMs (dW_r1, dW_r2, dW_o1, dW_o2) + 4 column sums; "
                   "lstm = tools/rollout_lstm_bench.py's rows of the same session and machine",
           "madds_per_sequence_step": {"interaction": madds_in(D, H), "lstm": madds_lstm(D, H)},
           "ratio_arithmetic": work, "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
