"""The whole step with the decoders' attention-window scale (PhysicsNet
``sigma=`` / ``log_sig``; reference physics_models.py:155-182).

spring_s12 at sigma = 2 (the one-CU decoder kernels), on the inputs and weights
of tests/golden/sigma/golden_spring_s12_sigma2.npz (the reference run with
log_sig = 2.0): constructor argument and attribute assignment, eager and
graph-captured, float and byte targets -- bit-identical to each other; outputs
and losses within 1e-4 of the fixture; every parameter gradient inside the fp32
envelope (tests/envelope.py: ENVELOPE_K times the spread of the reference
arithmetic's own fp32 runs around the float64 result) of the sigma-patched
float64 oracle.  Then log_sig 2 -> 1 reproduces golden_spring_s12 (no stale
graph or table), the eval-mode pass, conv_st_decoder / transf_masks, and the
range check.  3bp (K = 3, 36x36) and mnist (64x64) steps at sigma = 0.5 take the
generic decoder backward (9-wide gather window) end to end."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, load_golden, golden_weights, rel_err
from envelope import _record, _ulp_perturbed, ENSEMBLE, ENVELOPE_K, ENVELOPE_FLOOR, OUT_KEYS
from oracle import physics_oracle as O
import sigma_ref as SR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RT = 1e-4
ATTRS = {"enc_pos": "enc_pos", "enc_masks": "enc_masks", "recons_out": "recons_out", "output_seq": "output",
         "pos_vel_seq": "pos_vel_seq"}


def _fixture(name, log_sig):
    if log_sig == 2.0 and name == "spring_s12":
        return np.load(os.path.join(GOLDEN_DIR, "sigma", "golden_spring_s12_sigma2.npz"), allow_pickle=False)
    return load_golden(name)


@functools.lru_cache(maxsize=None)
def oracle_runs(name, log_sig):
    """envelope.oracle_runs under the sigma-patched oracle."""
    torch.set_num_threads(8)
    z = _fixture(name, log_sig)
    cfg, _ = O.cfg_from_golden(z)
    state = golden_weights(z)
    x = O.input_from_u8(z["input_u8"])
    with SR.patched_oracle(log_sig):
        f64 = _record(*O.train_step_f64(state, cfg, x))
        f32 = [_record(*O.train_step(state, cfg, x))]
        f32 += [_record(*O.train_step(_ulp_perturbed(state, s), cfg, x)) for s in range(ENSEMBLE)]
    return f64, f32


def _model(z, **kw):
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    task, cell, seq_len, ins, pred, size, B, ae, alt = [str(s) for s in z["config"]]
    torch.manual_seed(0)
    m = PhysicsNet(task, 100, 1, cell, int(seq_len), int(ins), int(pred), float(ae), bool(int(alt)), True,
                   int(size) ** 2, "conv_encoder", "conv_st_decoder", device=DEV, **kw).to(DEV)
    m.load_state_dict({k: v.to(DEV) for k, v in golden_weights(z).items()})
    return m


def _snapshot(m, loss):
    d = {k: getattr(m, a).detach().clone() for k, a in ATTRS.items()}
    d.update(loss_train=loss.detach().clone(), loss_extrap=m.extrap_loss.detach().clone(),
             loss_recons=m.recons_loss.detach().clone())
    d.update({"grad/" + n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    return d


def _graph_run(z, ctor, graph, byte_targets):
    """One step through GraphStep (lr = 0: every replay is the same step) on
    the fixture's sequences in dataset order; returns (snapshot, model, step)."""
    from paig_reproduction_amd.graph_step import GraphStep
    from paig_reproduction_amd.nn.datasets.iterators import DeviceDataIterator
    m = _model(z, sigma=2.0) if ctor else _model(z)
    if not ctor:
        m.log_sig = 2.0
    m.build_optimizer(0.0, "rmsprop", False)
    u8 = z["input_u8"]
    N, T, H = u8.shape[0], u8.shape[1], u8.shape[2]
    it = DeviceDataIterator(u8, (T, 3, H, H), DEV, seed=2)
    xbuf = torch.full((N, T, 3, H, H), float("nan"), device=DEV)
    gs = GraphStep(m, xbuf, 1, graph=graph)
    if byte_targets:
        gs.eng.byte_targets = it.bind_targets(xbuf, m.input_steps + m.pred_steps)
    it.next_batch(N, out=xbuf)
    loss = gs.eager()
    if graph:
        gs.capture()
        loss = gs()
    torch.cuda.synchronize()
    return _snapshot(m, loss), m, gs, xbuf


@functools.lru_cache(maxsize=None)
def _runs():
    z = _fixture("spring_s12", 2.0)
    return {(c, g, b): _graph_run(z, c, g, b) for c, g, b in
            ((True, False, False), (False, True, False), (True, False, True), (False, True, True))}


def _perm(xbuf, z):
    """Batch row -> fixture sequence."""
    x = O.input_from_u8(z["input_u8"]).to(xbuf.device)
    perm = [next(j for j in range(x.shape[0]) if torch.equal(xbuf[i, 0], x[j, 0])) for i in range(xbuf.shape[0])]
    assert sorted(perm) == list(range(x.shape[0]))
    return perm


def _rows(ref, perm):
    """A fixture array (sequence-major in its first axis) in the batch's row order."""
    B = len(perm)
    return ref.reshape(B, ref.shape[0] // B, *ref.shape[1:])[perm].reshape(ref.shape)


def test_sigma2_forms_bit_identical():
    runs = _runs()
    base = runs[(True, False, False)][0]
    for key, (snap, *_rest) in runs.items():
        assert set(snap) == set(base)
        bad = [k for k in base if not torch.equal(snap[k], base[k])]
        assert not bad, f"(ctor, graph, bytes) = {key}: {bad[:6]}"


def test_sigma2_matches_fixture_and_envelope():
    z = _fixture("spring_s12", 2.0)
    snap, m, gs, xbuf = _runs()[(True, False, False)]
    assert len(m.state_dict()) == 93 and m.log_sig == 2.0
    perm = _perm(xbuf, z)
    for k in ATTRS:
        ref = _rows(np.asarray(z[k]), perm)
        e = rel_err(snap[k].reshape(ref.shape), torch.from_numpy(ref))
        print(k, e)
        assert e <= RT, f"{k}: {e:.3g}"
    for k, zk in (("loss_train", "loss_train"), ("loss_extrap", "loss_extrap"), ("loss_recons", "loss_recons")):
        e = abs(float(snap[k]) - float(z[zk])) / abs(float(z[zk]))
        print(k, e)
        assert e <= RT, f"{k}: {e:.3g}"
    f64, f32 = oracle_runs("spring_s12", 2.0)
    over = {}
    for k in f64:
        if not k.startswith("grad/"):
            continue
        e_hip = rel_err(snap[k].double().cpu().numpy(), f64[k])
        e_32 = max(rel_err(r[k], f64[k]) for r in f32)
        bar = max(ENVELOPE_K * e_32, ENVELOPE_FLOOR)
        print(k, f"hip {e_hip:.2e} fp32 {e_32:.2e} bar {bar:.2e}")
        if e_hip > bar:
            over[k] = (e_hip, bar)
    assert not over, over
    assert sorted(k for k in snap if k.startswith("grad/")) == sorted(k for k in f64 if k.startswith("grad/"))


def test_switch_back_to_sigma1_recaptures():
    """log_sig 2 -> 1 on the graph-captured model: the next step is the
    sigma = 1 fixture's (same inputs and weights)."""
    z1 = load_golden("spring_s12")
    snap2, m, gs, xbuf = _runs()[(False, True, False)]
    perm = _perm(xbuf, z1)
    m.log_sig = 1.0
    loss = gs()
    torch.cuda.synchronize()
    assert gs.sigma == 1.0
    for k, a in ATTRS.items():
        ref = _rows(np.asarray(z1[k]), perm)
        assert rel_err(getattr(m, a).reshape(ref.shape), torch.from_numpy(ref)) <= RT, k
    assert abs(float(loss.detach()) - float(z1["loss_train"])) <= RT * abs(float(z1["loss_train"]))
    m.log_sig = 2.0   # and forth: the cached runs stay what they were
    loss = gs()
    torch.cuda.synchronize()
    assert torch.equal(loss, snap2["loss_train"]) and torch.equal(m.output, snap2["output_seq"])


def test_eval_pass_decoder_module_and_range():
    z = _fixture("spring_s12", 2.0)
    cfg, _ = O.cfg_from_golden(z)
    state = golden_weights(z)
    x = O.input_from_u8(z["input_u8"])
    m = _model(z, sigma=2.0)
    # the eval pass (eval_performance's body: eval mode, no_grad, forward + losses)
    m.eval()
    with torch.no_grad():
        m.output = m.conv_feedforward(x.to(DEV))
        _, (pred, extrap, recons) = m.compute_loss()
    with SR.patched_oracle(2.0):
        metrics, out = O.eval_metrics(state, cfg, x)
        assert rel_err(m.output, out["output_seq"]) <= RT
        for got, k in ((pred, "eval_pred_loss"), (extrap, "eval_extrap_loss"), (recons, "eval_recons_loss")):
            assert abs(float(got) - metrics[k]) <= RT * abs(metrics[k]), k
        # conv_st_decoder(pos) and its transf_* attributes
        m.train()
        pos = torch.from_numpy(np.asarray(z["enc_pos"]).reshape(-1, cfg.D).copy())
        pg = pos.to(DEV).requires_grad_(True)
        dec = m.conv_st_decoder(pg)
        joint, bg = O.decoder_sources(state, cfg)
        pr = pos.clone().requires_grad_(True)
        ref = O.st_decoder(cfg, joint, bg, pr)
        assert rel_err(dec, ref) <= RT
        rc, rm = O.st_decoder_parts(cfg, joint, bg, pos)
        for a, b in zip(list(m.transf_contents) + list(m.transf_masks), list(rc) + list(rm)):
            assert rel_err(a, b) <= RT
        R = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7))
        (dec * R.to(DEV)).sum().backward()
        (ref * R).sum().backward()
        assert rel_err(pg.grad, pr.grad) <= RT
    for bad in (4.0, 0.25, -1.0):
        m.log_sig = bad
        with pytest.raises(ValueError, match="sigma"):
            m(x.to(DEV))
        with pytest.raises(ValueError, match="sigma"):
            m.conv_st_decoder(pos.to(DEV))


@pytest.mark.parametrize("name", ["3bp_s20", "mnist_s12"])
def test_step_sigma_half(name):
    """sigma = 0.5: the window is twice the frame; the decoder backward of the
    one-CU shapes runs the generic kernels."""
    z = load_golden(name)
    m = _model(z)
    m.log_sig = 0.5
    x = O.input_from_u8(z["input_u8"]).to(DEV)
    m.output = m(x)
    loss, _ = m.compute_loss()
    m.zero_grad(set_to_none=True)
    loss.backward()
    torch.cuda.synchronize()
    snap = _snapshot(m, loss)
    f64, f32 = oracle_runs(name, 0.5)
    ref = f32[0]
    for k in OUT_KEYS:
        e = rel_err(snap[k].double().cpu().numpy().reshape(ref[k].shape), ref[k])
        print(k, e)
        assert e <= RT, f"{k}: {e:.3g}"
    for k in ("train", "extrap", "recons"):
        assert abs(float(snap["loss_" + k]) - ref["loss_" + k]) <= RT * abs(ref["loss_" + k]), k
    over = {}
    for k in f64:
        if not k.startswith("grad/"):
            continue
        e_hip = rel_err(snap[k].double().cpu().numpy(), f64[k])
        e_32 = max(rel_err(r[k], f64[k]) for r in f32)
        bar = max(ENVELOPE_K * e_32, ENVELOPE_FLOOR)
        print(k, f"hip {e_hip:.2e} fp32 {e_32:.2e} bar {bar:.2e}")
        if e_hip > bar:
            over[k] = (e_hip, bar)
    assert not over, over
