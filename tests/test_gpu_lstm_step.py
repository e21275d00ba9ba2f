"""The whole training step with the black-box cell (lstm_ode_cell, H = 100)
on the inputs and weights of the spring_s12 (D = 4, 32 x 32) and 3bp_s20
(D = 6, 36 x 36) fixtures, against the CPU oracle's step with the restated
cell of tests/rollout_lstm_ref.py added to its cell table for the test.
Outputs, losses and every gradient must lie within tests/envelope.py's rule
(ENVELOPE_K times the fp32 ensemble's own distance to float64).  Also an eval
forward at test_seq_len 30, the captured step against the eager one, and a
tiny --blackbox_dynamics train -> checkpoint -> test run of the CLI.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import envelope as E
import rollout_lstm_ref as LR
from helpers import golden_weights, load_golden, rel_err
from oracle import physics_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "runners"))
CELL = "lstm_ode_cell"
FIXTURES = ("spring_s12", "3bp_s20")
H = 100
LSTM_KEYS = tuple(LR.PFX + k for k in LR.KEYS)
_REF = {}   # fixture -> the restated cell the oracle steps with


@pytest.fixture
def oracle_lstm(monkeypatch):
    """The oracle's cell table with the restated cell and its six keys among
    the live parameters, for this test only."""
    def cell(P, pos, vel):
        return _REF["cell"](P, pos, vel)

    live = O.live_params

    def live_params(state, cfg):
        out = live(state, cfg)
        if cfg.cell == CELL:
            out.update({k: state[k] for k in LSTM_KEYS})
        return out

    monkeypatch.setattr(O, "CELLS", {**O.CELLS, CELL: cell})
    monkeypatch.setattr(O, "live_params", live_params)


def _state(z):
    """The fixture's weights with its physics cell's keys replaced by a seeded default LSTM cell's."""
    cfg, _ = O.cfg_from_golden(z)
    st = {k: v for k, v in golden_weights(z).items() if not k.startswith(LR.PFX)}
    st.update({LR.PFX + k: v for k, v in LR.default_weights(cfg.D, H, seed=11).items()})
    return st


def _oracle(fn, state, cfg, x, **kw):
    """One oracle step from a zero hidden state."""
    _REF["cell"] = LR.LstmCellRef(cfg.size / 2)
    _REF["cell"].reset()
    return fn(state, cfg, x, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_runs(name):
    """(fp64 result, [fp32 result, fp32 results on one-ulp-perturbed weights]); called under oracle_lstm."""
    torch.set_num_threads(8)
    z = load_golden(name)
    cfg, _ = O.cfg_from_golden(z)
    cfg.cell = CELL
    state = _state(z)
    x = O.input_from_u8(z["input_u8"])
    f64 = E._record(*_oracle(O.train_step_f64, state, cfg, x))
    f32 = [E._record(*_oracle(O.train_step, state, cfg, x))]
    f32 += [E._record(*_oracle(O.train_step, E._ulp_perturbed(state, s), cfg, x)) for s in range(E.ENSEMBLE)]
    return f64, f32


def _model(z, seq_len=None):
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    task, _, sl, ins, pred, size, B, ae, alt = [str(s) for s in z["config"]]
    torch.manual_seed(0)
    m = PhysicsNet(task, H, 1, CELL, seq_len or int(sl), int(ins), int(pred), float(ae), bool(int(alt)), True,
                   int(size) ** 2, "conv_encoder", "conv_st_decoder", device=DEV).to(DEV)
    m.load_state_dict({k: v.to(DEV) for k, v in _state(z).items()})   # strict
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


@pytest.mark.parametrize("name", FIXTURES)
def test_step_within_fp32_envelope(name, oracle_lstm):
    from test_gpu_parity import _input
    z = load_golden(name)
    f64, f32 = _oracle_runs(name)
    m = _model(z)
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
    # ---- not vacuous: the cell moves the objects and its gradients are non-zero
    pvs = hip["pos_vel_seq"]
    assert float(np.abs(pvs[:, 1:] - pvs[:, :1]).max()) > 1e-3
    for k in LSTM_KEYS:
        assert float(np.abs(hip["grad/" + k]).max()) > 0 and float(np.abs(f64["grad/" + k]).max()) > 0, k
    _envelope(name, hip, f64, f32)


@pytest.mark.parametrize("name", FIXTURES)
def test_eval_forward_at_test_seq_len(name, oracle_lstm):
    """no_grad forward over 30 frames (the null-workspace path, R = 26)."""
    z = load_golden(name)
    cfg, _ = O.cfg_from_golden(z)
    cfg30 = O.Cfg(cfg.task, CELL, 30, cfg.input_steps, cfg.pred_steps, cfg.size, cfg.ae, cfg.alt_vel)
    x = O.input_from_u8(z["input_u8"])
    x30 = torch.cat([x, x.flip(1), x], 1)[:2, :30].contiguous()
    state = _state(z)
    torch.set_num_threads(8)

    def rec(out, L, g):
        return {k: out[k].detach().double().numpy() for k in E.OUT_KEYS}

    f64 = rec(*_oracle(O.train_step_f64, state, cfg30, x30, with_grads=False))
    f32 = [rec(*_oracle(O.train_step, state, cfg30, x30, with_grads=False))]
    f32 += [rec(*_oracle(O.train_step, E._ulp_perturbed(state, s), cfg30, x30, with_grads=False))
            for s in range(E.ENSEMBLE)]
    m = _model(z, seq_len=30).eval()
    with torch.no_grad():
        out = m(x30.to(DEV))
    torch.cuda.synchronize()
    assert out.shape[1] == 30 - cfg.input_steps
    hip = {"enc_pos": m.enc_pos, "enc_masks": m.enc_masks, "recons_out": m.recons_out, "output_seq": out,
           "pos_vel_seq": m.pos_vel_seq}
    _envelope(name + "@30", {k: v.detach().double().cpu().numpy() for k, v in hip.items()}, f64, f32)


def _snapshot(m, loss):
    d = {"loss": loss.detach().clone(), "pos_vel_seq": m.pos_vel_seq.detach().clone(), "output": m.output.detach().clone()}
    d.update({"grad/" + n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    return d


def test_captured_step_equals_eager_step():
    """lr = 0: every replay is the same step.  The cell's workspace comes from
    the caching allocator, so the capture needs nothing special."""
    from paig_reproduction_amd.graph_step import GraphStep
    from test_gpu_parity import _input
    z = load_golden("spring_s12")
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
            for _ in range(2):
                loss = gs()
                torch.cuda.synchronize()
                snaps.append(_snapshot(m, loss))
    base = snaps[0]
    assert all("grad/" + k in base for k in LSTM_KEYS)
    for i, s in enumerate(snaps[1:]):
        assert set(s) == set(base)
        bad = [k for k in base if not torch.equal(s[k], base[k])]
        assert not bad, f"snapshot {i + 1}: {bad[:6]}"


def test_module_call_is_step_one_of_the_fused_rollout():
    from test_gpu_parity import _input
    z = load_golden("spring_s12")
    m = _model(z)
    with torch.no_grad():
        m.output = m(_input(z, DEV))
    pvs = m.pos_vel_seq.detach()
    D = pvs.shape[2] // 2
    p1, v1 = m.rollout_cell(pvs[:, 0, :D].contiguous(), pvs[:, 0, D:].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(p1, pvs[:, 1, :D]) and torch.equal(v1, pvs[:, 1, D:])


@pytest.fixture
def torch_logger():
    import logging
    lg = logging.getLogger("torch")
    handlers, level = list(lg.handlers), lg.level
    yield lg
    for h in list(lg.handlers):
        if h not in handlers:
            lg.removeHandler(h)
    lg.setLevel(level)


def test_cli_blackbox_train_then_test(tmp_path, torch_logger):
    import torch_run_physics as R
    save = str(tmp_path / "run")
    data = str(tmp_path / "data")
    common = ["--task", "spring_color", "--blackbox_dynamics", "--color", "--autoencoder_loss", "3.0",
              "--batch_size", "20", "--save_dir", save, "--data_dir", data, "--synthetic", "200", "--seed", "4"]
    net = R.main(common + ["--epochs", "1", "--save_every_n_epochs", "1", "--print_interval", "1"])
    assert net.cell_type == CELL and net.rollout_cell.recurrent_units == 100
    ckpt = os.path.join(save, "model.ckpt")
    assert os.path.exists(ckpt)
    out = np.load(os.path.join(save, "outputs.npz"))
    assert out["input"].shape[1:] == (30, 3, 32, 32)           # test_seq_len
    assert np.isfinite(out["output"]).all()
    assert bool(torch.isfinite(net.pos_vel_seq.detach()).all())
    import re
    for loss in (net.pred_loss, net.extrap_loss, net.recons_loss):
        assert bool(torch.isfinite(loss.detach()).all())
    log = open(os.path.join(save, "log.txt")).read()
    assert re.search(r"loss", log, re.I) and not re.search(r"\b(nan|inf)\b", log, re.I), log[-2000:]
    # its own checkpoint reloads strictly into a fresh black-box model
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    sd = torch.load(ckpt, map_location="cpu")
    sd = sd.get("model", sd.get("state_dict", sd)) if isinstance(sd, dict) else sd
    fresh = PhysicsNet("spring_color", 100, 1, CELL, 12, 4, 6, 3.0, False, True, 32 * 32, "conv_encoder",
                       "conv_st_decoder", device=DEV)
    fresh.load_state_dict(sd, strict=True)
    assert all(k in sd for k in LSTM_KEYS)
