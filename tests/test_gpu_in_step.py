"""The whole training step with the interaction-network cell
(interaction_ode_cell, H = 100 and H = 12) on the inputs and weights of the
spring_s12 (D = 4, 32 x 32) and 3bp_s20 (D = 6, 36 x 36) fixtures, against the
CPU oracle's step with the restated cell of tests/rollout_in_ref.py added to
its cell table for the test.  Outputs, losses and every gradient must lie
within tests/envelope.py's rule (ENVELOPE_K times the fp32 ensemble's own
distance to float64), the bars tests/test_gpu_lstm_step.py uses.  Also an eval
forward at test_seq_len 30, the captured step against the eager one, the cell
called on its own, and a tiny --interaction_dynamics train -> checkpoint ->
test run of the CLI.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import envelope as E
import rollout_in_ref as IR
from helpers import golden_weights, load_golden, rel_err
from oracle import physics_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "runners"))
CELL = "interaction_ode_cell"
FIXTURES = ("spring_s12", "3bp_s20")
WIDTHS = (100, 12)
IN_KEYS = tuple(IR.PFX + k for k in IR.KEYS)
_REF = {}   # the restated cell the oracle steps with


@pytest.fixture
def oracle_in(monkeypatch):
    """The oracle's cell table with the restated cell and its eight keys among
    the live parameters, for this test only."""
    def cell(P, pos, vel):
        return _REF["cell"](P, pos, vel)

    live = O.live_params

    def live_params(state, cfg):
        out = live(state, cfg)
        if cfg.cell == CELL:
            out.update({k: state[k] for k in IN_KEYS})
        return out

    monkeypatch.setattr(O, "CELLS", {**O.CELLS, CELL: cell})
    monkeypatch.setattr(O, "live_params", live_params)


def _state(z, H):
    """The fixture's weights with its physics cell's keys replaced by a seeded default interaction cell's."""
    cfg, _ = O.cfg_from_golden(z)
    st = {k: v for k, v in golden_weights(z).items() if not k.startswith(IR.PFX)}
    st.update({IR.PFX + k: v for k, v in IR.default_weights(cfg.D, H, seed=11).items()})
    return st


def _oracle(fn, state, cfg, x, **kw):
    _REF["cell"] = IR.InCellRef(cfg.size / 2)
    return fn(state, cfg, x, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_runs(name, H):
    """(fp64 result, [fp32 result, fp32 results on one-ulp-perturbed weights]); called under oracle_in."""
    torch.set_num_threads(8)
    z = load_golden(name)
    cfg, _ = O.cfg_from_golden(z)
    cfg.cell = CELL
    state = _state(z, H)
    x = O.input_from_u8(z["input_u8"])
    f64 = E._record(*_oracle(O.train_step_f64, state, cfg, x))
    f32 = [E._record(*_oracle(O.train_step, state, cfg, x))]
    f32 += [E._record(*_oracle(O.train_step, E._ulp_perturbed(state, s), cfg, x)) for s in range(E.ENSEMBLE)]
    return f64, f32


def _model(z, H=100, seq_len=None):
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    task, _, sl, ins, pred, size, B, ae, alt = [str(s) for s in z["config"]]
    torch.manual_seed(0)
    m = PhysicsNet(task, H, 1, CELL, seq_len or int(sl), int(ins), int(pred), float(ae), bool(int(alt)), True,
                   int(size) ** 2, "conv_encoder", "conv_st_decoder", device=DEV).to(DEV)
    m.load_state_dict({k: v.to(DEV) for k, v in _state(z, H).items()})   # strict
    return m


def _envelope(tag, hip, f64, f32):
    over, worst = {}, (0.0, None)
    for k in f64:
        if k == "loss_pred":
            continue
        assert k in hip, f"{k}: no such output / gradient from the HIP step"
        e = rel_err(np.asarray(hip[k]), np.asarray(f64[k]))
        e32 = max(rel_err(np.asarray(r[k]), np.asarray(f64[k])) for r in f32)
        bar = max(E.ENVELOPE_K * e32, E.ENVELOPE_FLOOR)
        print(f"ENVELOPE {tag} {k:44s} hip {e:.2e}  e32 {e32:.2e}  bar {bar:.2e}")
        if not e <= bar:
            over[k] = f"hip {e:.2e} > {E.ENVELOPE_K:g} x fp32 {e32:.2e}"
        worst = max(worst, (e / bar, k))
    print(tag, "worst hip/bar:", worst)
    assert not over, over


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("name", FIXTURES)
def test_step_within_fp32_envelope(name, H, oracle_in):
    from test_gpu_parity import _input
    z = load_golden(name)
    f64, f32 = _oracle_runs(name, H)
    m = _model(z, H)
    m.output = m(_input(z, DEV))
    train_loss, (pred, extrap, recons) = m.compute_loss()
    m.zero_grad(set_to_none=True)
    train_loss.backward()
    torch.cuda.synchronize()
    hip = {"enc_pos": m.enc_pos, "enc_masks": m.enc_masks, "recons_out": m.recons_out, "output_seq": m.output,
           "pos_vel_seq": m.pos_vel_seq}
    hip = {k: v.detach().double().cpu().numpy() for k, v in hip.items()}
    hip.update(loss_train=float(train_loss.detach()), loss_extrap=float(extrap.detach()), loss_recons=float(recons.detach()))
    for k, p in m.named_parameters():
        if p.grad is not None:
            hip["grad/" + k] = p.grad.detach().double().cpu().numpy()
    # ---- not vacuous: the cell moves the objects and its gradients are non-zero, in p.grad through the flat buffer
    pvs = hip["pos_vel_seq"]
    assert float(np.abs(pvs[:, 1:] - pvs[:, :1]).max()) > 1e-3
    for k in IN_KEYS:
        assert float(np.abs(hip["grad/" + k]).max()) > 0 and float(np.abs(f64["grad/" + k]).max()) > 0, k
    _envelope(f"{name} H={H}", hip, f64, f32)


@pytest.mark.parametrize("name", FIXTURES)
def test_eval_forward_at_test_seq_len(name, oracle_in, monkeypatch):
    """no_grad forward over 30 frames (the null-workspace path, R = 26): no
    workspace is allocated, and the frames of the shared prefix match the
    training-length forward's."""
    z = load_golden(name)
    cfg, _ = O.cfg_from_golden(z)
    cfg30 = O.Cfg(cfg.task, CELL, 30, cfg.input_steps, cfg.pred_steps, cfg.size, cfg.ae, cfg.alt_vel)
    x = O.input_from_u8(z["input_u8"])
    x30 = torch.cat([x, x.flip(1), x], 1)[:2, :30].contiguous()
    state = _state(z, 100)
    torch.set_num_threads(8)

    def rec(out, L, g):
        return {k: out[k].detach().double().numpy() for k in E.OUT_KEYS}

    f64 = rec(*_oracle(O.train_step_f64, state, cfg30, x30, with_grads=False))
    f32 = [rec(*_oracle(O.train_step, state, cfg30, x30, with_grads=False))]
    f32 += [rec(*_oracle(O.train_step, E._ulp_perturbed(state, s), cfg30, x30, with_grads=False))
            for s in range(E.ENSEMBLE)]
    m = _model(z, seq_len=30).eval()
    from paig_reproduction_amd._lib import lib
    asked = []
    real = lib().paig_rollout_in_workspace
    with monkeypatch.context() as mp:   # the engine sizes the workspace with this call, and only when it allocates one
        mp.setattr(lib(), "paig_rollout_in_workspace", lambda *a: asked.append(a) or real(*a), raising=False)
        with torch.no_grad():
            out = m(x30.to(DEV))
        torch.cuda.synchronize()
    assert not asked, "an inference forward asked for the cell's workspace"
    assert out.shape[1] == 30 - cfg.input_steps
    hip = {"enc_pos": m.enc_pos, "enc_masks": m.enc_masks, "recons_out": m.recons_out, "output_seq": out,
           "pos_vel_seq": m.pos_vel_seq}
    _envelope(name + "@30", {k: v.detach().double().cpu().numpy() for k, v in hip.items()}, f64, f32)
    # the training-length forward (with a workspace) on the same sequences: the shared prefix
    T = cfg.seq_len
    mt = _model(z)
    with monkeypatch.context() as mp:
        mp.setattr(lib(), "paig_rollout_in_workspace", lambda *a: asked.append(a) or real(*a), raising=False)
        mt.output = mt(x30[:, :T].contiguous().to(DEV))
        torch.cuda.synchronize()
    assert len(asked) == 1, "a training forward allocates the cell's workspace once"
    # (the encoder's dynamic operand scales see another set of frames, so not bit for bit: both forwards must
    # lie within the envelope of the float64 step's prefix)
    for k, t in (("output_seq", mt.output), ("pos_vel_seq", mt.pos_vel_seq)):
        n = t.shape[1]
        e32 = max(rel_err(r[k][:, :n], f64[k][:, :n]) for r in f32)
        bar = max(E.ENVELOPE_K * e32, E.ENVELOPE_FLOOR)
        for tag, got in (("train", t), ("eval", getattr(m, "pos_vel_seq") if k == "pos_vel_seq" else out)):
            e = rel_err(got.detach().double().cpu().numpy()[:, :n], f64[k][:, :n])
            print(f"PREFIX {name} {k} {tag} {e:.2e} bar {bar:.2e}")
            assert e <= bar, (k, tag, e, bar)


def _snapshot(m, loss):
    d = {"loss": loss.detach().clone(), "pos_vel_seq": m.pos_vel_seq.detach().clone(), "output": m.output.detach().clone()}
    d.update({"grad/" + n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    return d


def test_captured_step_equals_eager_step():
    """lr = 0: every replay is the same step.  The cell's workspace comes from
    the caching allocator, so the capture needs nothing special."""
    from paig_reproduction_amd.graph_step import GraphStep
    from test_gpu_parity import _input
    z = load_golden("3bp_s20")
    snaps = []
    for graph in (False, True):
        m = _model(z)
        m.build_optimizer(0.0, "rmsprop", False)
        xbuf = _input(z, DEV).contiguous()
        gs = GraphStep(m, xbuf, 1, graph=graph)
        loss = gs.eager()
        torch.cuda.synchronize()
        snaps.append(_snapshot(m, loss))
        if graph:
            gs.capture()
            for _ in range(3):
                loss = gs()
                torch.cuda.synchronize()
                snaps.append(_snapshot(m, loss))
    base = snaps[0]
    assert all("grad/" + k in base for k in IN_KEYS)
    assert len(snaps) == 5
    for i, s in enumerate(snaps[1:]):
        assert set(s) == set(base)
        bad = [k for k in base if not torch.equal(s[k], base[k])]
        assert not bad, f"snapshot {i + 1}: {bad[:6]}"


@pytest.mark.parametrize("name", FIXTURES)
def test_module_call_is_one_step_of_the_restatement(name):
    from test_gpu_parity import _input
    z = load_golden(name)
    m = _model(z)
    with torch.no_grad():
        m.output = m(_input(z, DEV))
    pvs = m.pos_vel_seq.detach()
    D = pvs.shape[2] // 2
    pos, vel = pvs[:, 0, :D].contiguous(), pvs[:, 0, D:].contiguous()
    p1, v1 = m.rollout_cell(pos, vel)
    torch.cuda.synchronize()
    # step one of the fused rollout, bit for bit
    assert torch.equal(p1, pvs[:, 1, :D]) and torch.equal(v1, pvs[:, 1, D:])
    # and the restatement's step within the fp32 envelope of its own ensemble
    W = IR.default_weights(D, 100, seed=11)
    half = m.rollout_cell.half

    def step(W, dtype):
        P = {k: v.to(dtype) for k, v in W.items()}
        p, v = IR.InCellRef(half, prefix="")(P, pos.cpu().to(dtype), vel.cpu().to(dtype))
        return torch.cat([p, v], 1).double().numpy()

    f64 = step(W, torch.float64)
    e32 = max(rel_err(step(w, torch.float32), f64) for w in [W] + [E._ulp_perturbed(W, s) for s in range(E.ENSEMBLE)])
    got = torch.cat([p1, v1], 1).detach().double().cpu().numpy()
    assert rel_err(got, f64) <= max(E.ENVELOPE_K * e32, E.ENVELOPE_FLOOR)
    # its autograd path deposits the eight parameter gradients
    m.zero_grad(set_to_none=True)
    pos.requires_grad_(True)
    p2, v2 = m.rollout_cell(pos, vel)
    (p2.sum() + v2.sum()).backward()
    torch.cuda.synchronize()
    assert pos.grad is not None and float(pos.grad.abs().max()) > 0
    for k, p in m.rollout_cell.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, k


def test_cli_interaction_train_then_test(tmp_path):
    """A fresh child process: one epoch of --interaction_dynamics training on
    synthetic data, its log, its outputs and its checkpoint."""
    import re
    import subprocess
    save = str(tmp_path / "run")
    data = str(tmp_path / "data")
    cmd = [sys.executable, os.path.join(REPO, "runners", "torch_run_physics.py"), "--task", "spring_color",
           "--interaction_dynamics", "--color", "--autoencoder_loss", "3.0", "--batch_size", "20", "--save_dir", save,
           "--data_dir", data, "--synthetic", "200", "--seed", "4", "--epochs", "1", "--save_every_n_epochs", "1",
           "--print_interval", "1"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    ckpt = os.path.join(save, "model.ckpt")
    assert os.path.exists(ckpt)
    out = np.load(os.path.join(save, "outputs.npz"))
    assert out["input"].shape[1:] == (30, 3, 32, 32)           # test_seq_len
    assert np.isfinite(out["output"]).all()
    log = open(os.path.join(save, "log.txt")).read()
    assert re.search(r"loss", log, re.I) and not re.search(r"\b(nan|inf)\b", log, re.I), log[-2000:]
    # its checkpoint reloads strictly into a fresh test-time model of the cell
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    sd = torch.load(ckpt, map_location="cpu")
    sd = sd.get("model", sd.get("state_dict", sd)) if isinstance(sd, dict) else sd
    fresh = PhysicsNet("spring_color", 100, 1, CELL, 30, 4, 6, 3.0, False, True, 32 * 32, "conv_encoder",
                       "conv_st_decoder", device=DEV)
    fresh.load_state_dict(sd, strict=True)
    assert all(k in sd for k in IN_KEYS)
