"""The whole step with the learnable attention-window scale
(``PhysicsNet(learn_sigma=True)``: sigma = exp(ln 2 tanh(decoder_sigma_u)),
formed, used and trained on the device), on the spring_s12 fixture.

  * at a start of sigma = 1 the forward is the fixed model's bit for bit, and
    every other parameter's gradient meets the fixture bars of
    test_gpu_parity.py (the decoder backward is the generic kernel, so no bit
    equality there);
  * at a start of sigma = 1.5: d loss / du inside the fp32 envelope
    (tests/envelope.py's rule) of the float64 oracle, whose decoder is
    tests/sigma_grad_ref.py so that sigma carries a gradient; every other
    gradient at the fixture bar against the fp32 run of that oracle;
  * 94 / 93 state_dict keys, flat offsets of the existing parameters unchanged;
  * three RMSprop steps eager, captured, and captured with the optimizer in
    the graph: bit-identical, u moving at every step, one capture;
  * a torch.save / load(weights_only=True) round trip restores sigma exactly;
  * the runner's --learn_sigma.
"""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

from helpers import load_golden, golden_weights, rel_err, grad_checks, RTOL
from envelope import _record, _ulp_perturbed, ENSEMBLE, ENVELOPE_K, ENVELOPE_FLOOR
from oracle import physics_oracle as O
import sigma_grad_ref as SG
from test_gpu_parity import GRAD_RTOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ATTRS = ("enc_pos", "enc_masks", "recons_out", "output", "pos_vel_seq")


def _model(z, **kw):
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    task, cell, seq_len, ins, pred, size, B, ae, alt = [str(s) for s in z["config"]]
    torch.manual_seed(0)
    m = PhysicsNet(task, 100, 1, cell, int(seq_len), int(ins), int(pred), float(ae), bool(int(alt)), True,
                   int(size) ** 2, "conv_encoder", "conv_st_decoder", device=DEV, **kw).to(DEV)
    m.load_state_dict({k: v.to(DEV) for k, v in golden_weights(z).items()}, strict=False)
    return m


def _step(m, x):
    m.output = m(x)
    loss, _ = m.compute_loss()
    m.zero_grad(set_to_none=True)
    loss.backward()
    torch.cuda.synchronize()
    snap = {a: getattr(m, a).detach().clone() for a in ATTRS}
    snap.update(loss_train=loss.detach().clone(), loss_extrap=m.extrap_loss.detach().clone(),
                loss_recons=m.recons_loss.detach().clone())
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    return snap, grads


def test_start_at_one_is_the_fixed_model_and_layout():
    z = load_golden("spring_s12")
    x = O.input_from_u8(z["input_u8"]).to(DEV)
    fixed = _model(z)
    fixed._native()
    offsets = dict(fixed._flat.index)
    assert len(fixed.state_dict()) == 93 and "decoder_sigma_u" not in dict(fixed.named_parameters())
    s0, g0 = _step(fixed, x)
    learn = _model(z, sigma=1.0, learn_sigma=True)
    assert len(learn.state_dict()) == 94 and float(learn.decoder_sigma_u.detach()) == 0.0
    s1, g1 = _step(learn, x)
    assert learn.decoder_sigma() == 1.0
    bad = [k for k in s0 if not torch.equal(s0[k], s1[k])]
    assert not bad, bad
    # the new slot is the fp32 buffer's last; every other parameter where it was
    idx = dict(learn._flat.index)
    u = idx.pop("decoder_sigma_u")
    assert idx == offsets and u == (32, fixed._flat.n32, 1, ()) and learn._flat.n32 == fixed._flat.n32 + 1
    assert learn._flat.n32_early == fixed._flat.n32_early
    again = _model(z)   # a default model built after the learnable one: the same layout, no new parameter
    again._native()
    assert dict(again._flat.index) == offsets and "decoder_sigma_u" not in dict(again.named_parameters())
    # gradients: everything the fixed model has, at the fixture bars, plus u's
    assert sorted(g1) == sorted(list(g0) + ["decoder_sigma_u"])
    assert torch.isfinite(g1["decoder_sigma_u"]).all() and float(g1["decoder_sigma_u"]) != 0.0
    grad_checks(z, {k: v for k, v in g1.items() if k != "decoder_sigma_u"}, GRAD_RTOL, prefix="learn_sigma: ")


@functools.lru_cache(maxsize=None)
def _oracle_runs(u32):
    """(float64 record, fp32 records) of the spring_s12 step with sigma =
    exp(ln 2 tanh(u)), u a leaf: each record carries grad/decoder_sigma_u."""
    torch.set_num_threads(8)
    z = load_golden("spring_s12")
    cfg, _ = O.cfg_from_golden(z)
    state = golden_weights(z)
    x = O.input_from_u8(z["input_u8"])

    def run(step, st, dtype):
        u = torch.tensor(float(u32), dtype=dtype, requires_grad=True)
        with SG.patched_oracle(SG.sigma_from_u(u)):
            rec = _record(*step(st, cfg, x))
        rec["grad/decoder_sigma_u"] = u.grad.detach().double().numpy()
        return rec

    f64 = run(O.train_step_f64, state, torch.float64)
    f32 = [run(O.train_step, state, torch.float32)]
    f32 += [run(O.train_step, _ulp_perturbed(state, s), torch.float32) for s in range(ENSEMBLE)]
    return f64, f32


def test_start_at_one_and_a_half_gradients():
    z = load_golden("spring_s12")
    x = O.input_from_u8(z["input_u8"]).to(DEV)
    m = _model(z, sigma=1.5, learn_sigma=True)
    u32 = float(m.decoder_sigma_u.detach())
    snap, grads = _step(m, x)
    f64, f32 = _oracle_runs(u32)
    ref = f32[0]
    for a, k in zip(ATTRS, ("enc_pos", "enc_masks", "recons_out", "output_seq", "pos_vel_seq")):
        e = rel_err(snap[a].double().cpu().numpy().reshape(ref[k].shape), ref[k])
        assert e <= RTOL, f"{k}: {e:.3g}"
    for k in ("train", "extrap", "recons"):
        assert abs(float(snap["loss_" + k]) - ref["loss_" + k]) <= RTOL * abs(ref["loss_" + k]), k
    # d loss / du: the envelope rule against float64
    k = "grad/decoder_sigma_u"
    assert abs(float(f64[k])) > 0
    e_hip = rel_err(grads["decoder_sigma_u"].double().cpu().numpy(), f64[k])
    e_32 = max(rel_err(r[k], f64[k]) for r in f32)
    bar = max(ENVELOPE_K * e_32, ENVELOPE_FLOOR)
    print(f"d loss/du: hip {float(grads['decoder_sigma_u']):.9g} f64 {float(f64[k]):.9g} "
          f"err {e_hip:.2e} fp32 {e_32:.2e} bar {bar:.2e}")
    assert e_hip <= bar, (e_hip, bar)
    # every other gradient at the fixture bar, against the fp32 run of the same oracle
    keys = sorted(n for n in grads if n != "decoder_sigma_u")
    assert keys == sorted(q[len("grad/"):] for q in ref if q.startswith("grad/") and q != k)
    for n in keys:
        e = rel_err(grads[n].double().cpu().numpy(), ref["grad/" + n])
        assert e <= GRAD_RTOL, f"grad {n}: {e:.3g}"


def _train3(mode):
    from paig_reproduction_amd.graph_step import GraphStep
    z = load_golden("spring_s12")
    m = _model(z, sigma=1.5, learn_sigma=True)
    m.build_optimizer(1e-3, "rmsprop", False)
    xbuf = O.input_from_u8(z["input_u8"]).to(DEV).contiguous()
    gs = GraphStep(m, xbuf, 1, graph=mode != "eager", optimizer_in_graph=mode == "graph+opt")
    us = [float(m.decoder_sigma_u.detach())]
    gs.eager()
    us.append(float(m.decoder_sigma_u.detach()))
    gs.capture()
    for _ in range(2):
        gs()
        torch.cuda.synchronize()
        us.append(float(m.decoder_sigma_u.detach()))
    gs.finish()
    assert gs.opt_in_graph == (mode == "graph+opt")
    return {n: p.detach().clone() for n, p in m.named_parameters()}, us, gs.captures, m


def test_three_rmsprop_steps_eager_captured_and_optimizer_in_graph():
    runs = {mode: _train3(mode) for mode in ("eager", "graph", "graph+opt")}
    base, us, _, _ = runs["eager"]
    assert len(set(us)) == 4, us                      # u moves at every step
    for mode, (params, u, captures, m) in runs.items():
        assert captures == (0 if mode == "eager" else 1), (mode, captures)
        assert u == us, (mode, u, us)
        bad = [n for n in base if not torch.equal(params[n], base[n])]
        assert not bad, (mode, bad[:6])
        assert 0.5 < m.decoder_sigma() < 2.0


def test_state_dict_round_trip_and_errors(tmp_path):
    z = load_golden("spring_s12")
    params, us, _, m = _train3("graph+opt")
    path = str(tmp_path / "model.ckpt")
    torch.save(m.state_dict(), path)
    sd = torch.load(path, weights_only=True)
    assert len(sd) == 94 and "decoder_sigma_u" in sd
    fresh = _model(z, learn_sigma=True)
    fresh.load_state_dict(sd)
    assert fresh.decoder_sigma() == m.decoder_sigma() and fresh.decoder_sigma() != 1.0
    assert torch.equal(fresh.decoder_sigma_u.detach(), m.decoder_sigma_u.detach())
    with pytest.raises(ValueError, match="sigma"):
        _model(z, sigma=2.0, learn_sigma=True)
    with pytest.raises(AttributeError, match="decoder_sigma_u"):
        m.log_sig = 1.0


def test_standalone_decoder_uses_and_trains_the_learned_sigma():
    """conv_st_decoder / transf_* in learnable mode: the learned sigma in the
    forward, u's gradient deposited by the backward (the step's kernels)."""
    import types
    z = load_golden("spring_s12")
    cfg, _ = O.cfg_from_golden(z)
    state = golden_weights(z)
    m = _model(z, sigma=1.5, learn_sigma=True)
    pos = torch.from_numpy(np.asarray(z["enc_pos"]).reshape(-1, cfg.D).copy())
    dec = m.conv_st_decoder(pos.to(DEV).requires_grad_(True))
    joint, bg = O.decoder_sources(state, cfg)
    u = m.decoder_sigma_u.detach().cpu().clone().requires_grad_(True)
    sg = SG.sigma_from_u(u)
    ref = SG.st_decoder_sigma(cfg, joint, bg, pos, sg)
    assert rel_err(dec, ref) <= RTOL
    rc, rm = SG.st_decoder_parts_sigma(cfg, joint, bg, pos, sg.detach())
    for a, b in zip(list(m.transf_contents) + list(m.transf_masks), list(rc) + list(rm)):
        assert rel_err(a, b) <= RTOL
    R = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7))
    m.zero_grad(set_to_none=True)
    (dec * R.to(DEV)).sum().backward()
    (ref * R).sum().backward()
    assert rel_err(m.decoder_sigma_u.grad.reshape(()), u.grad.reshape(())) <= GRAD_RTOL


def test_runner_learn_sigma(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "runners"))
    import torch_run_physics as R
    lg = logging.getLogger("torch")
    handlers, level = list(lg.handlers), lg.level
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())

    keep = Keep(level=logging.DEBUG)
    lg.addHandler(keep)
    try:
        save, data = str(tmp_path / "run"), str(tmp_path / "data")
        net = R.main(["--task", "spring_color", "--color", "--autoencoder_loss", "3.0", "--epochs", "1",
                      "--batch_size", "10", "--save_dir", save, "--save_every_n_epochs", "1", "--print_interval", "1",
                      "--data_dir", data, "--synthetic", "40", "--seed", "0", "--learn_sigma", "--sigma", "1.2"])
    finally:
        for h in list(lg.handlers):
            if h not in handlers:
                lg.removeHandler(h)
        lg.setLevel(level)
    sd = torch.load(os.path.join(save, "model.ckpt"), weights_only=True)
    assert len(sd) == 94 and "decoder_sigma_u" in sd
    train = [ln for ln in lines if ln.startswith("train - iter=")]
    assert train and all("decoder_sigma=" in ln for ln in train), train[:2]
    assert net.learn_sigma and torch.equal(net.decoder_sigma_u.detach().cpu(), sd["decoder_sigma_u"].cpu())
