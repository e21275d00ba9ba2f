#!/usr/bin/env python3
"""Cost of the learnable decoder window scale (PhysicsNet(learn_sigma=True))
at the headline shape: spring_color, B = 100, seq 50, the step captured in a
HIP graph with the optimizer inside (bench.py's workload).

Alternates learn_sigma off / on in one process (ROUNDS rounds of STEPS timed
replays each, device events per step, the median reported), then times the
two decoder backward launches per mode with the engine's kernel probe over
eager steps: off = the one-CU kernels, on = the generic kernel (every frame
walked, three barriers per frame) plus its dL/dsigma sums.

    python tools/learn_sigma_cost.py [--rounds 3] [--steps 50] [--batch 100]

Prints one JSON line.  Needs the GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def build(learn, a, dev):
    from paig_reproduction_amd.graph_step import GraphStep
    from paig_reproduction_amd.nn.datasets.iterators import DeviceDataIterator
    from paig_reproduction_amd.nn.datasets.synth import render_sequences
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    torch.manual_seed(0)
    m = PhysicsNet("spring_color", 100, 1, "spring_ode_cell", a.seq_len, 4, 6, 3.0, False, True, 32 * 32,
                   "conv_encoder", "conv_st_decoder", device=dev, learn_sigma=learn).to(dev)
    m.build_optimizer(6e-4, "rmsprop", True)
    u8 = render_sequences("spring_color", 64, a.seq_len, seed=1)
    u8 = np.concatenate([u8] * max(1, -(-8 * a.batch // 64)), 0)
    it = DeviceDataIterator(u8, (a.seq_len, 3, 32, 32), dev, seed=0)
    xbuf = torch.empty((a.batch, a.seq_len, 3, 32, 32), device=dev)
    gs = GraphStep(m, xbuf, 1, graph=True, optimizer_in_graph=True)
    gs.eng.byte_targets = it.bind_targets(xbuf, 10)

    def eager():
        it.next_batch(a.batch, out=xbuf)
        return gs.eager()

    for _ in range(a.warmup):
        eager()
    gs.capture()

    def step():
        it.next_batch(a.batch, out=xbuf)
        return gs()

    step()
    torch.cuda.synchronize()
    return m, gs, step, eager


def timed(step, n):
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    evs[0].record()
    for i in range(n):
        step()
        evs[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(n))
    return per[n // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--seq_len", type=int, default=50)
    ap.add_argument("--probe_steps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("learn_sigma_cost: needs the GPU (no CPU fallback)")
    from paig_reproduction_amd import engine as E
    dev = torch.device("cuda:0")
    runs = {learn: build(learn, a, dev) for learn in (False, True)}
    med = {False: [], True: []}
    for _ in range(a.rounds):
        for learn in (False, True):
            med[learn].append(round(timed(runs[learn][2], a.steps), 4))
    kern = {}
    for learn, (m, gs, step, eager) in runs.items():
        probe = E.KernelProbe(None)
        gs.eng.probe = probe
        for _ in range(a.probe_steps):
            eager()
        gs.eng.probe = None
        s = probe.summaries()
        kern[learn] = {t: round(s[t]["avg_ms"] * 1e3, 2) for t in ("dec_bwd:rollout", "dec_bwd:recon", "dec_fwd:rollout")
                       if t in s}
    off, on = float(np.median(med[False])), float(np.median(med[True]))
    print(json.dumps({"workload": f"spring_color B={a.batch} seq={a.seq_len} graph+optimizer",
                      "step_ms_off": med[False], "step_ms_on": med[True], "median_off": off, "median_on": on,
                      "on_over_off": round(on / off, 4), "kernel_us_off": kern[False], "kernel_us_on": kern[True],
                      "sigma_after": runs[True][0].decoder_sigma()}))


if __name__ == "__main__":
    main()
