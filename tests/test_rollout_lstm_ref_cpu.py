"""CPU checks of the black-box rollout cell: the restatement the GPU tests use
as their reference (tests/rollout_lstm_ref.py) against real nn.LSTMCell /
nn.Linear modules and torch.autograd.gradcheck, the cell's state_dict, its
constructor's validation and the --blackbox_dynamics flag.  No GPU."""
import os
import sys

import pytest
import torch

import rollout_lstm_ref as LR

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "runners"))


def _inputs(B, D, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    pos = 4 + 24 * torch.rand(B, D, generator=g, dtype=torch.float64)
    vel = -3 + 6 * torch.rand(B, D, generator=g, dtype=torch.float64)
    return pos.to(dtype), vel.to(dtype)


@pytest.mark.parametrize("B,D,H,R,half", [(3, 4, 12, 5, 16.0), (2, 6, 20, 4, 18.0)])
def test_restatement_equals_torch_modules_f64(B, D, H, R, half):
    W = {k: v.double() for k, v in LR.default_weights(D, H, seed=1).items()}
    pos, vel = _inputs(B, D, 2)
    got = LR.rollout(W, pos, vel, R, half)
    lstm, proj = torch.nn.LSTMCell(2 * D, H).double(), torch.nn.Linear(H, 2 * D).double()
    with torch.no_grad():
        lstm.weight_ih.copy_(W["lstm.weight_ih"]), lstm.weight_hh.copy_(W["lstm.weight_hh"])
        lstm.bias_ih.copy_(W["lstm.bias_ih"]), lstm.bias_hh.copy_(W["lstm.bias_hh"])
        proj.weight.copy_(W["proj.weight"]), proj.bias.copy_(W["proj.bias"])
        h = c = torch.zeros(B, H, dtype=torch.float64)
        p, v = pos, vel
        seq = [torch.cat([p, v], 1)]
        for _ in range(R):
            h, c = lstm(torch.cat([(p - half) / half, v / half], 1), (h, c))
            y = proj(h)
            p, v = p + half * y[:, :D], v + half * y[:, D:]
            seq.append(torch.cat([p, v], 1))
    want = torch.stack(seq, 1)
    assert got.shape == (B, R + 1, 2 * D)
    assert float((got - want).abs().max()) <= 1e-12
    assert float((got[:, 1:] - got[:, :1]).abs().max()) > 1e-3   # the cell moves the objects


def test_restatement_carries_state_and_resets():
    D, H = 4, 8
    W = {LR.PFX + k: v.double() for k, v in LR.default_weights(D, H, seed=3).items()}
    pos, vel = _inputs(2, D, 4)
    cell = LR.LstmCellRef(16.0)
    a1 = cell(W, pos, vel)
    a2 = cell(W, pos, vel)      # carried h, c: another result from the same inputs
    cell.reset()
    b1 = cell(W, pos, vel)
    assert torch.equal(a1[0], b1[0]) and torch.equal(a1[1], b1[1])
    assert not torch.equal(a1[0], a2[0])


def test_restatement_gradcheck():
    B, D, H, R = 2, 4, 4, 2
    W = {k: v.double().requires_grad_(True) for k, v in LR.default_weights(D, H, seed=5).items()}
    pos, vel = _inputs(B, D, 6)
    pos.requires_grad_(True), vel.requires_grad_(True)

    def f(pos, vel, *ws):
        return LR.rollout(dict(zip(LR.KEYS, ws)), pos, vel, R, 16.0)

    assert torch.autograd.gradcheck(f, (pos, vel, *[W[k] for k in LR.KEYS]), eps=1e-6, atol=1e-6)


def _net(cell_type, **kw):
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    args = dict(task="spring_color", recurrent_units=100, lstm_layers=1, cell_type=cell_type, seq_len=12, input_steps=4,
                pred_steps=6, autoencoder_loss=3.0, color=True, input_size=32 * 32, encoder_type="conv_encoder")
    args.update(kw)
    return PhysicsNet(**args)


@pytest.mark.parametrize("task,size,H", [("spring_color", 32, 100), ("3bp_color", 36, 12)])
def test_cell_state_dict(task, size, H):
    torch.manual_seed(0)
    m = _net("lstm_ode_cell", task=task, input_size=size * size, recurrent_units=H)
    D = m.coord_units // 2
    from paig_reproduction_amd.nn.network.cells import lstm_ode_cell, ode_cell
    assert type(m.rollout_cell) is lstm_ode_cell and not isinstance(m.rollout_cell, ode_cell)
    assert m.rollout_cell.half == size / 2
    sd = m.state_dict()
    cell = {k[len(LR.PFX):]: v for k, v in sd.items() if k.startswith(LR.PFX)}
    assert {k: tuple(v.shape) for k, v in cell.items()} == LR.key_shapes(D, H)
    assert all(v.dtype == torch.float32 for v in cell.values())
    # the six names are live, in the rollout branch's bucket and the "physics" gradient-norm group
    live = [n for n in m._live_names() if n.startswith(LR.PFX)]
    assert live == [LR.PFX + k for k in LR.KEYS]
    from paig_reproduction_amd.flat import FlatParams
    assert all(FlatParams.group_of(n) == "physics" and n.startswith(m.ROLLOUT_PARAMS) for n in live)
    assert not any(n.startswith(m.EARLY_GRADS) for n in live)
    # every other key as the default model's for the same seed
    torch.manual_seed(0)
    ref = _net({"spring_color": "spring_ode_cell", "3bp_color": "gravity_ode_cell"}[task], task=task,
               input_size=size * size).state_dict()
    other = [k for k in sd if not k.startswith(LR.PFX)]
    assert other == [k for k in ref if not k.startswith(LR.PFX)]
    assert all(torch.equal(sd[k], ref[k]) for k in other)
    # the read-out is the default draw scaled by 0.1
    assert float(sd[LR.PFX + "proj.weight"].abs().max()) <= 0.1 / H ** 0.5 + 1e-7


@pytest.mark.parametrize("H", [0, 2, 6, 132, 256, 10])
def test_hidden_width_validation(H):
    with pytest.raises(ValueError):
        _net("lstm_ode_cell", recurrent_units=H)


def test_layers_validation_and_the_lstm_key():
    with pytest.raises(ValueError):
        _net("lstm_ode_cell", lstm_layers=2)
    with pytest.raises(NotImplementedError, match="lstm_ode_cell"):
        _net("lstm")
    for H in (4, 128):
        _net("lstm_ode_cell", recurrent_units=H)


def test_blackbox_flag():
    import torch_run_physics as R
    p = R.build_parser()
    assert p.parse_args(["--task", "spring_color"]).blackbox_dynamics is False
    for task, (_, _, preset, *_rest) in R.TASKS.items():
        assert R.task_cell(p.parse_args(["--task", task, "--blackbox_dynamics"])) == "lstm_ode_cell"
        assert R.task_cell(p.parse_args(["--task", task])) == preset
    assert len(R.TASKS) == 5
    with pytest.raises(SystemExit):
        R.task_cell(p.parse_args(["--task", "spring_color", "--blackbox_dynamics", "--physics_2d"]))
