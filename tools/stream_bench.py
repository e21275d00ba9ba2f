"""Cost of streaming fresh training batches (StreamingDeviceIterator) against
the resident dataset (DeviceDataIterator), on the step bench.py times: the
GraphStep replay with byte targets bound.

Per configuration it reports
  * the device time of one refill (draw -> integrate -> compact -> raster), HIP
    events on the refill stream of an otherwise idle device;
  * the step time with the resident and with the streaming iterator, in
    alternating blocks of one process: each round times resident, resident
    again (the A/A pair: the noise) and streaming;
  * the stream's statistics (accepted per refill, shortfall slots).
The check: streaming <= resident + refill + A/A spread.  The first two terms
are a refill that hides behind nothing; more than that means something blocks
the host or the compute stream.

    PYTHONPATH=. python tools/stream_bench.py --out profiles/synth_stream.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.realpath(__file__)), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# task: (cell, ins, pred, size) -- bench.py TASKS
TASKS = {"spring_color": ("spring_ode_cell", 4, 6, 32), "bouncing_balls": ("bouncing_ode_cell", 4, 6, 32),
         "3bp_color": ("gravity_ode_cell", 4, 12, 36), "mnist_spring_color": ("spring_ode_cell", 3, 7, 64)}
CONFIGS = (("spring_color", 100, 50), ("bouncing_balls", 1024, 100))


def block(step, steps):
    """``steps`` steps between two events: (device ms per step, host ms per step)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) * 1e3 / steps


def run(task, B, T, a, dev):
    from paig_reproduction_amd.graph_step import GraphStep
    from paig_reproduction_amd.nn.datasets.iterators import DeviceDataIterator, StreamingDeviceIterator
    from paig_reproduction_amd.nn.datasets.synth_device import render_sequences_device
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    cell, ins, pred, size = TASKS[task]
    torch.manual_seed(0)
    m = PhysicsNet(task, 100, 1, cell, T, ins, pred, a.ae, False, True, size * size, "conv_encoder", "conv_st_decoder",
                   device=dev).to(dev)
    m.conv_math = "split"
    m.build_optimizer(a.lr, "rmsprop", True)
    xbuf = torch.empty((B, T, 3, size, size), device=dev)
    u8 = render_sequences_device(task, 2 * B, T, seed=1, device=dev).repeat(a.dataset // 2, 1, 1, 1, 1)
    its = {"resident": DeviceDataIterator(u8, (T, 3, size, size), dev, seed=0),
           "streaming": StreamingDeviceIterator(task, T, B, dev, epoch_size=a.dataset * B, seed=0)}
    steps = {}
    for name, it in its.items():   # one captured step per iterator: the byte targets' base is a graph constant
        gs = GraphStep(m, xbuf, 1, graph=True)
        gs.eng.byte_targets = it.bind_targets(xbuf, ins + pred)
        for _ in range(a.warmup):
            it.next_batch(B, out=xbuf)
            gs.eager()
        gs.capture()

        def step(it=it, gs=gs):
            it.next_batch(B, out=xbuf)
            return gs()

        for _ in range(a.warmup):
            step()
        steps[name] = step
    dev_ms = {"resident": [], "resident_again": [], "streaming": []}
    host_ms = {k: [] for k in dev_ms}
    for _ in range(a.rounds):
        for key in ("resident", "resident_again", "streaming"):
            d, h = block(steps["streaming" if key == "streaming" else "resident"], a.steps)
            dev_ms[key].append(d)
            host_ms[key].append(h)
    stats = its["streaming"].stats()

    # one refill alone, on a third iterator nobody reads
    probe = StreamingDeviceIterator(task, T, B, dev, epoch_size=a.dataset * B, seed=1)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.refills + 1)]
    ev[0].record(probe.refill_stream)
    for i in range(a.refills):
        probe._refill(i % 2, 2 + i)
        ev[i + 1].record(probe.refill_stream)
    torch.cuda.synchronize()
    refill = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.refills))

    res_all = dev_ms["resident"] + dev_ms["resident_again"]
    resident, streaming = statistics.median(res_all), statistics.median(dev_ms["streaming"])
    refill_ms = statistics.median(refill)
    aa = max(abs(x - y) for x, y in zip(dev_ms["resident"], dev_ms["resident_again"]))
    out = {"task": task, "batch": B, "seq_len": T, "steps_per_block": a.steps, "rounds": a.rounds,
           "resident_step_ms": resident, "streaming_step_ms": streaming, "refill_ms": refill_ms,
           "refill_ms_min_max": [refill[0], refill[-1]], "aa_spread_ms": aa,
           "bound_ms": resident + refill_ms + aa, "within_bound": streaming <= resident + refill_ms + aa,
           "blocks_device_ms": dev_ms, "blocks_host_ms": host_ms, "candidates": stats["candidates"],
           "accepted_per_refill": stats["accepted_per_refill"], "refills": stats["refills"],
           "shortfall_slots": stats["shortfall_slots"], "pool_bytes": int(its["streaming"].X.numel())}
    del steps, its, probe, m, xbuf, u8
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=100, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=4, help="resident / resident / streaming rounds")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--refills", type=int, default=20, help="refills timed alone")
    ap.add_argument("--dataset", type=int, default=8, help="resident dataset (and nominal epoch) in batches")
    ap.add_argument("--ae", type=float, default=3.0)
    ap.add_argument("--lr", type=float, default=6e-4)
    ap.add_argument("--config", action="append", default=None, metavar="TASK:BATCH:SEQ_LEN",
                    help="default: spring_color:100:50 and bouncing_balls:1024:100")
    ap.add_argument("--out", default=None, help="write the JSON here too")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench measures on the GPU only")
    cfgs = CONFIGS if not a.config else [(t, int(b), int(s)) for t, b, s in (c.split(":") for c in a.config)]
    dev = torch.device("cuda:0")
    res = {"tool": "tools/stream_bench.py", "device": torch.cuda.get_device_name(0),
           "configs": [run(t, b, s, a, dev) for t, b, s in cfgs]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
