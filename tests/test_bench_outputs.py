"""bench.py's plain run, --full and --dump-outputs.

CPU tests: a plain run switches off everything the headline figure does not
need (roofline probes, config legs, CPU baseline) and --full leaves their
own switches as given; dump_outputs writes fp32 / fp64 .npy files, a large
array as the same seeded sample every time, and refuses more than 64 MB.
GPU test: one small plain run with --dump-outputs, whose line must hold the
headline keys with empty --full fields, and whose files must be the step's
outputs (finite, fp32 / fp64, loss equal to the line's final_loss).
"""
import glob
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _parse(monkeypatch, args):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + args)
    return bench.parse()


def test_plain_run_has_no_full_only_work(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.legs, a.cpu_baseline, a.probe_steps) == (False, 0, 0, 0)
    assert (a.steps, a.warmup, a.dump_outputs) == (7, 2, None)
    # the switches of the moved parts do nothing without --full
    a = _parse(monkeypatch, ["--legs", "1", "--cpu_baseline", "1", "--probe_steps", "3"])
    assert (a.legs, a.cpu_baseline, a.probe_steps) == (0, 0, 0)


def test_full_keeps_the_switches(monkeypatch):
    a = _parse(monkeypatch, ["--full"])
    assert (a.full, a.legs, a.cpu_baseline, a.probe_steps) == (True, 1, 1, 5)
    a = _parse(monkeypatch, ["--full", "--legs", "0", "--cpu_baseline", "0", "--probe_steps", "2",
                             "--dump-outputs", "d"])
    assert (a.legs, a.cpu_baseline, a.probe_steps, a.dump_outputs) == (0, 0, 2, "d")


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, ["--steps", "0"])


def test_dump_outputs_formats_and_sample(tmp_path):
    big = torch.arange(bench.DUMP_SAMPLE + 7, dtype=torch.float32).reshape(-1, 1)
    t = {"loss": torch.tensor(1.5), "g": torch.tensor(2.0, dtype=torch.float64),
         "h": torch.ones(3, 2, dtype=torch.bfloat16).float().half(), "big": big}
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(d1, t)
    bench.dump_outputs(d2, {"big": big + 1})
    got = {os.path.basename(p)[:-4]: np.load(p) for p in glob.glob(os.path.join(d1, "*.npy"))}
    assert sorted(got) == ["big", "g", "h", "loss"]
    assert got["loss"].dtype == np.float32 and got["loss"].shape == () and got["loss"] == 1.5
    assert got["g"].dtype == np.float64 and got["g"] == 2.0
    assert got["h"].dtype == np.float32 and got["h"].shape == (3, 2)
    s = got["big"]
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(s) > 0) and s[-1] <= bench.DUMP_SAMPLE + 6   # distinct elements of the array, in order
    # the same elements in every run
    assert np.array_equal(np.load(os.path.join(d2, "big.npy")), s + 1)


def test_dump_outputs_refuses_more_than_the_limit(tmp_path):
    n = bench.DUMP_LIMIT // (4 * bench.DUMP_SAMPLE)   # sampled arrays that fill the limit exactly
    big = torch.zeros(bench.DUMP_SAMPLE + 1)
    t = {f"a{i}": big for i in range(n)}
    bench.dump_outputs(str(tmp_path / "ok"), t)
    t["one_more"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "over"), t)


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    d = str(tmp_path / "out")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-u", os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--batch", "4", "--seq_len", "12", "--dataset", "2", "--dump-outputs", d],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["full"] is False and line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "video-seqs/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # value is the sequences of the timed steps over their time
    assert math.isclose(line["value"], 4 / (line["ms_per_step"] * 1e-3), rel_tol=1e-2)
    assert line["legs"] == {} and line["cpu_baseline"] is None and line["roofline"] is None
    assert line["roofline_headline"] is None and line["roofline_others"] == {} and line["hbm_step"] is None
    got = {os.path.basename(p)[:-4]: np.load(p) for p in glob.glob(os.path.join(d, "*.npy"))}
    for k in ("loss", "extrap_loss", "recons_loss", "output_seq", "recons_out", "enc_pos", "pos_vel_seq",
              "param.encoder.l1.weight", "grad.encoder.l1.weight"):
        assert k in got, sorted(got)
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), (k, v.dtype)
        assert np.isfinite(v).all(), k
    assert got["output_seq"].size == 4 * 8 * 3 * 32 * 32     # 12 - 4 input steps rolled out
    assert got["recons_out"].size == 4 * 10 * 3 * 32 * 32    # 4 input + 6 prediction steps reconstructed
    assert got["param.encoder.l1.weight"].shape == got["grad.encoder.l1.weight"].shape
    assert np.abs(got["grad.encoder.l1.weight"]).max() > 0
    assert math.isclose(float(got["loss"]), line["final_loss"], rel_tol=1e-3, abs_tol=1e-4)
