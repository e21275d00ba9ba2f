"""CPU checks of the interaction-network rollout cell: the restatement the GPU
tests use as their reference (tests/rollout_in_ref.py) against the cell's own
nn.Sequential modules composed by hand and torch.autograd.gradcheck, its
permutation equivariance, the cell's state_dict, its constructor's validation
and the --interaction_dynamics flag.  No GPU."""
import os
import sys

import pytest
import torch

import rollout_in_ref as IR

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "runners"))


def _inputs(B, D, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    pos = 4 + 24 * torch.rand(B, D, generator=g, dtype=torch.float64)
    vel = -3 + 6 * torch.rand(B, D, generator=g, dtype=torch.float64)
    return pos.to(dtype), vel.to(dtype)


@pytest.mark.parametrize("B,D,H,R,half", [(3, 4, 12, 5, 16.0), (2, 6, 20, 4, 18.0)])
def test_restatement_equals_cell_modules_f64(B, D, H, R, half):
    from paig_reproduction_amd.nn.network.cells import interaction_ode_cell
    torch.manual_seed(1)
    cell = interaction_ode_cell(D, D, H, half).double()
    W = {k: v.detach() for k, v in cell.state_dict().items()}
    assert tuple(W) == IR.KEYS and {k: tuple(v.shape) for k, v in W.items()} == IR.key_shapes(D, H)
    pos, vel = _inputs(B, D, 2)
    got = IR.rollout(W, pos, vel, R, half)
    K = D // 2
    with torch.no_grad():
        p, v = pos, vel
        seq = [torch.cat([p, v], 1)]
        for _ in range(R):
            s = [torch.cat([(p[:, 2 * i:2 * i + 2] - half) / half, v[:, 2 * i:2 * i + 2] / half], 1) for i in range(K)]
            np_, nv_ = [], []
            for i in range(K):
                a = sum(cell.rel(torch.cat([s[i], s[j]], 1)) for j in range(K) if j != i)
                y = cell.obj(torch.cat([s[i], a], 1))
                np_.append(p[:, 2 * i:2 * i + 2] + half * y[:, :2])
                nv_.append(v[:, 2 * i:2 * i + 2] + half * y[:, 2:])
            p, v = torch.cat(np_, 1), torch.cat(nv_, 1)
            seq.append(torch.cat([p, v], 1))
    want = torch.stack(seq, 1)
    assert got.shape == (B, R + 1, 2 * D)
    assert float((got - want).abs().max()) <= 1e-12
    assert float((got[:, 1:] - got[:, :1]).abs().max()) > 1e-3   # the cell moves the objects


@pytest.mark.parametrize("B,D,H,R", [(3, 4, 8, 2), (2, 6, 8, 2)])
def test_restatement_gradcheck(B, D, H, R):
    W = {k: v.double().requires_grad_(True) for k, v in IR.default_weights(D, H, seed=5).items()}
    pos, vel = _inputs(B, D, 6)
    pos.requires_grad_(True), vel.requires_grad_(True)

    def f(pos, vel, *ws):
        return IR.rollout(dict(zip(IR.KEYS, ws)), pos, vel, R, 16.0 if D == 4 else 18.0)

    assert torch.autograd.gradcheck(f, (pos, vel, *[W[k] for k in IR.KEYS]), eps=1e-6, atol=1e-6)


@pytest.mark.parametrize("perm", [(1, 0, 2), (2, 0, 1), (2, 1, 0)])
def test_permutation_equivariance_f64(perm):
    B, D, H, R = 4, 6, 20, 5
    W = {k: v.double() for k, v in IR.default_weights(D, H, seed=9).items()}
    pos, vel = _inputs(B, D, 10)
    idx = torch.tensor([2 * i + c for i in perm for c in (0, 1)])
    out = IR.rollout(W, pos, vel, R, 18.0)
    outp = IR.rollout(W, pos[:, idx], vel[:, idx], R, 18.0)
    full = torch.cat([idx, D + idx])
    assert float((outp - out[:, :, full]).abs().max()) <= 1e-12
    assert float((out[:, :, full] - out).abs().max()) > 1e-3   # the permutation moves something


def _net(cell_type, **kw):
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    args = dict(task="spring_color", recurrent_units=100, lstm_layers=1, cell_type=cell_type, seq_len=12, input_steps=4,
                pred_steps=6, autoencoder_loss=3.0, color=True, input_size=32 * 32, encoder_type="conv_encoder")
    args.update(kw)
    return PhysicsNet(**args)


@pytest.mark.parametrize("task,size,H", [("spring_color", 32, 100), ("3bp_color", 36, 12)])
def test_cell_state_dict(task, size, H):
    torch.manual_seed(0)
    m = _net("interaction_ode_cell", task=task, input_size=size * size, recurrent_units=H)
    D = m.coord_units // 2
    from paig_reproduction_amd.nn.network.cells import interaction_ode_cell, ode_cell
    assert type(m.rollout_cell) is interaction_ode_cell and not isinstance(m.rollout_cell, ode_cell)
    assert m.rollout_cell.KIND == 6 and m.rollout_cell.half == size / 2
    sd = m.state_dict()
    cell = {k[len(IR.PFX):]: v for k, v in sd.items() if k.startswith(IR.PFX)}
    assert {k: tuple(v.shape) for k, v in cell.items()} == IR.key_shapes(D, H)
    assert all(v.dtype == torch.float32 for v in cell.values())
    # the eight names are live, after every other name, in the rollout branch's bucket and the "physics" group
    names = m._live_names()
    live = [n for n in names if n.startswith(IR.PFX)]
    assert live == [IR.PFX + k for k in IR.KEYS] and names[-len(live):] == live
    from paig_reproduction_amd.flat import FlatParams
    assert all(FlatParams.group_of(n) == "physics" and n.startswith(m.ROLLOUT_PARAMS) for n in live)
    assert not any(n.startswith(m.EARLY_GRADS) for n in live)
    # every other key as the default model's for the same seed
    torch.manual_seed(0)
    ref = _net({"spring_color": "spring_ode_cell", "3bp_color": "gravity_ode_cell"}[task], task=task,
               input_size=size * size).state_dict()
    other = [k for k in sd if not k.startswith(IR.PFX)]
    assert other == [k for k in ref if not k.startswith(IR.PFX)]
    assert all(torch.equal(sd[k], ref[k]) for k in other)
    # the last object layer is the default draw scaled by 0.1
    assert float(sd[IR.PFX + "obj.2.weight"].abs().max()) <= 0.1 / H ** 0.5 + 1e-7
    assert float(sd[IR.PFX + "obj.2.bias"].abs().max()) <= 0.1 / H ** 0.5 + 1e-7


@pytest.mark.parametrize("H", [0, 2, 6, 132, 256, 10, True, 8.0])
def test_hidden_width_validation(H):
    from paig_reproduction_amd.nn.network.cells import interaction_ode_cell
    with pytest.raises(ValueError):
        interaction_ode_cell(4, 4, H, 16.0)


def test_hidden_width_bounds_build():
    from paig_reproduction_amd.nn.network.cells import interaction_ode_cell
    for H in (4, 128):
        assert interaction_ode_cell(6, 6, H, 18.0).recurrent_units == H


def test_interaction_flag():
    import torch_run_physics as R
    p = R.build_parser()
    assert p.parse_args(["--task", "spring_color"]).interaction_dynamics is False
    for task, (_, _, preset, *_rest) in R.TASKS.items():
        assert R.task_cell(p.parse_args(["--task", task, "--interaction_dynamics"])) == "interaction_ode_cell"
        assert R.task_cell(p.parse_args(["--task", task, "--blackbox_dynamics"])) == "lstm_ode_cell"
        assert R.task_cell(p.parse_args(["--task", task])) == preset
    with pytest.raises(SystemExit):
        R.task_cell(p.parse_args(["--task", "spring_color", "--interaction_dynamics", "--physics_2d"]))
    with pytest.raises(SystemExit):
        R.task_cell(p.parse_args(["--task", "spring_color", "--interaction_dynamics", "--blackbox_dynamics"]))
