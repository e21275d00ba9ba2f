"""The whole training step with the opt-in 2-D cells (spring2d_ode_cell,
bouncing2d_ode_cell) on the inputs and weights of the spring_s12 /
bouncing_s12 fixtures, against the CPU oracle's step with the restated cells
of tests/rollout2d_cases.py (split size 2) added to its cell table for the
test.  Outputs, losses and every gradient must lie within tests/envelope.py's
rule (ENVELOPE_K times the fp32 ensemble's own distance to float64), as in
test_gpu_envelope.py.  Also the one-step module call, and a tiny
--physics_2d train -> checkpoint -> test run of the CLI.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import envelope as E
import rollout2d_cases as C2
from helpers import golden_weights, load_golden, rel_err
from oracle import physics_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "runners"))
CASES = {"spring2d_ode_cell": "spring_s12", "bouncing2d_ode_cell": "bouncing_s12"}
CELLS_2D = {"spring2d_ode_cell": lambda P, pos, vel: C2.spring_cell(P, pos, vel, 2),
            "bouncing2d_ode_cell": lambda P, pos, vel: C2.bouncing_cell(P, pos, vel, 2)}


@pytest.fixture
def oracle_2d(monkeypatch):
    """The oracle's cell table with the two restated 2-D cells, for this test only."""
    monkeypatch.setattr(O, "CELLS", {**O.CELLS, **CELLS_2D})


@functools.lru_cache(maxsize=None)
def _oracle_runs(cell):
    """envelope.oracle_runs with the fixture's cell replaced by ``cell``: (fp64
    result, [fp32 result, fp32 results on one-ulp-perturbed weights]).  Called
    under the oracle_2d fixture."""
    torch.set_num_threads(8)
    z = load_golden(CASES[cell])
    cfg, _ = O.cfg_from_golden(z)
    cfg.cell = cell
    state = golden_weights(z)
    x = O.input_from_u8(z["input_u8"])
    f64 = E._record(*O.train_step_f64(state, cfg, x))
    f32 = [E._record(*O.train_step(state, cfg, x))]
    f32 += [E._record(*O.train_step(E._ulp_perturbed(state, s), cfg, x)) for s in range(E.ENSEMBLE)]
    return f64, f32


def _model(z, cell):
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    task, _, seq_len, ins, pred, size, B, ae, alt = [str(s) for s in z["config"]]
    torch.manual_seed(0)
    m = PhysicsNet(task, 100, 1, cell, int(seq_len), int(ins), int(pred), float(ae), bool(int(alt)), True,
                   int(size) ** 2, "conv_encoder", "conv_st_decoder", device=DEV).to(DEV)
    m.load_state_dict({k: v.to(DEV) for k, v in golden_weights(z).items()})   # strict: the 1-D fixture's keys
    return m


def _hip_step(z, cell):
    """The HIP step on the fixture's weights / inputs with ``cell``: ({key: float64 numpy}, model)."""
    from test_gpu_parity import _input
    m = _model(z, cell)
    m.output = m(_input(z, DEV))
    train_loss, (pred, extrap, recons) = m.compute_loss()
    m.zero_grad(set_to_none=True)
    train_loss.backward()
    torch.cuda.synchronize()
    d = {"enc_pos": m.enc_pos, "enc_masks": m.enc_masks, "recons_out": m.recons_out, "output_seq": m.output,
         "pos_vel_seq": m.pos_vel_seq}
    d = {k: v.detach().double().cpu().numpy() for k, v in d.items()}
    d.update(loss_train=float(train_loss.detach()), loss_extrap=float(extrap.detach()), loss_recons=float(recons.detach()))
    for k, p in m.named_parameters():
        if p.grad is not None:
            d["grad/" + k] = p.grad.detach().double().cpu().numpy()
    return d, m


@pytest.mark.parametrize("cell", list(CASES))
def test_step_within_fp32_envelope(cell, oracle_2d):
    z = load_golden(CASES[cell])
    f64, f32 = _oracle_runs(cell)
    hip, m = _hip_step(z, cell)
    # ---- guards against a vacuous pass
    pvs = hip["pos_vel_seq"]
    assert float(np.abs(pvs[:, 1:, 2:4] - pvs[:, :1, 2:4]).max()) > 1e-3, "object 1 does not move over the rollout"
    one_d, _ = _hip_step(z, cell.replace("2d", ""))
    assert float(np.abs(one_d["pos_vel_seq"] - pvs).max()) > 1e-3, "the 2-D rollout is the 1-D model's"
    if cell == "spring2d_ode_cell":
        for k in ("grad/rollout_cell.k", "grad/rollout_cell.equil"):
            assert abs(float(hip[k])) > 0 and abs(float(f64[k])) > 0, k
    else:
        assert not any(k.startswith("grad/rollout_cell.") for k in hip)
    # ---- the envelope rule on every output, loss and gradient
    over, worst = {}, (0.0, None)
    for k in f64:
        if k == "loss_pred":
            continue
        assert k in hip, f"{k}: no such output / gradient from the HIP step"
        e = rel_err(np.asarray(hip[k]), np.asarray(f64[k]))
        e32 = max(rel_err(np.asarray(r[k]), np.asarray(f64[k])) for r in f32)
        bar = max(E.ENVELOPE_K * e32, E.ENVELOPE_FLOOR)
        print(f"ENVELOPE {cell} {k:44s} hip {e:.2e}  e32 {e32:.2e}  bar {bar:.2e}")
        if not e <= bar:
            over[k] = f"hip {e:.2e} > {E.ENVELOPE_K:g} x fp32 {e32:.2e}"
        worst = max(worst, (e / bar, k))
    print(cell, "worst hip/bar:", worst)
    assert not over, over


@pytest.mark.parametrize("cell", list(CASES))
def test_module_call_is_step_one_of_the_fused_rollout(cell):
    """rollout_cell(pos, vel) (paig_rollout_fwd with R = 1) gives the fused
    rollout's first step bit for bit."""
    z = load_golden(CASES[cell])
    from test_gpu_parity import _input
    m = _model(z, cell)
    with torch.no_grad():
        m.output = m(_input(z, DEV))
    pvs = m.pos_vel_seq.detach()
    D = pvs.shape[2] // 2
    p1, v1 = m.rollout_cell(pvs[:, 0, :D].contiguous(), pvs[:, 0, D:].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(p1, pvs[:, 1, :D]) and torch.equal(v1, pvs[:, 1, D:])
    assert float((p1[:, 2:4] - pvs[:, 0, 2:4]).abs().max()) > 0


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


def test_cli_physics_2d_train_then_test(tmp_path, torch_logger):
    """test_cli_train_then_test's run with --physics_2d.  Seed 4, not that
    test's 0: at seeds 0, 2 and 3 the fresh model's two ReLU'd mask logits are
    zero at every pixel (quirk Q13), both objects get exactly the same
    position, and the reference's own arithmetic (the CPU oracle with the
    restated split-size-2 cell, fp32 autograd) has a non-finite gradient at
    n = 0 in its first step; at seeds 1, 4 and 5 the oracle's gradient is
    finite (4: both logits alive).  The seed was chosen by that CPU result."""
    import torch_run_physics as R
    save = str(tmp_path / "run")
    data = str(tmp_path / "data")
    net = R.main(["--task", "spring_color", "--physics_2d", "--color", "--autoencoder_loss", "3.0", "--epochs", "2",
                  "--batch_size", "10", "--save_dir", save, "--save_every_n_epochs", "1", "--print_interval", "1",
                  "--data_dir", data, "--synthetic", "40", "--seed", "4"])
    assert net.cell_type == "spring2d_ode_cell" and type(net.rollout_cell).KIND == 3
    assert os.path.exists(os.path.join(save, "model.ckpt"))
    out = np.load(os.path.join(save, "outputs.npz"))
    assert out["input"].shape[1:] == (30, 3, 32, 32)           # test_seq_len
    assert np.isfinite(out["output"]).all()
    assert net.output.shape[1] == 30 - 4
    pvs = net.pos_vel_seq.detach().cpu()
    assert bool(torch.isfinite(pvs).all())
    assert float((pvs[:, 1:, 2:4] - pvs[:, :1, 2:4]).abs().max()) > 1e-3, "object 1's predicted positions are constant"
