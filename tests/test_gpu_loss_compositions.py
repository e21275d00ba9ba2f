"""Every loss a caller can build from compute_loss()'s outputs, through the
whole training step (the suite otherwise only backpropagates train_loss):

  train, extrap, recons, train + 0.5 extrap, extrap + 3 recons,
  0.7 train + 1.3 extrap + 2.1 recons

on spring_s12 (ShallowUNet, 32x32, 2 extrapolation steps) and 3bp_s20 (36x36,
gravity, K = 3).

1. Against the oracle: the same scalar built from O.forward + O.losses
   (whose train already includes ae * recons), fp32 CPU autograd.  Bars per
   key: the fp32 envelope as test_gpu_modules._envelope_bars forms it,
   max(ENVELOPE_K x the spread of the oracle on one-ulp-perturbed weights,
   1e-4) -- measured on the oracle, not on the code under test.  One oracle
   forward per ensemble member serves all six compositions.
2. The in-kernel loss weights against the weight arrays
   (PAIG_LOSSW_INKERNEL=0): bit-identical gradients.
3. Two backwards in sequence on one model with different compositions: the
   second matches a fresh model's (nothing of the first survives).
4. Two same-shaped models under one backward: each gets its own loss's
   gradients.
5. compute_loss() called twice on one forward, terms of both in the loss.

Dead-value guard: a composition's oracle gradients of the var_net_* weights
(and of the physics parameter, where a rollout term is present) must be
non-zero, or a comparison of zeros with zeros could pass; keys whose oracle
gradient is identically zero must be exactly zero on the device."""
import functools

import pytest
import torch

from helpers import load_golden, golden_weights, rel_err, worst_err
from envelope import ENVELOPE_K, _ulp_perturbed
from oracle import physics_oracle as O
from test_gpu_parity import _model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RT = 1e-4
MEMBERS = 10
FIXTURES = ["spring_s12", "3bp_s20"]
PHYS = {"spring_s12": "rollout_cell.k", "3bp_s20": "rollout_cell.g"}
# name -> (weights of train, extrap, recons)
COMPS = {
    "train": (1.0, 0.0, 0.0),
    "extrap": (0.0, 1.0, 0.0),
    "recons": (0.0, 0.0, 1.0),
    "train+0.5extrap": (1.0, 0.5, 0.0),
    "extrap+3recons": (0.0, 1.0, 3.0),
    "0.7train+1.3extrap+2.1recons": (0.7, 1.3, 2.1),
}


def _compose(coef, train, extrap, recons):
    """The scalar, built only from the terms present (an absent term is not
    in the graph at all, as when a caller never touches it)."""
    total = None
    for c, t in zip(coef, (train, extrap, recons)):
        if c != 0.0:
            term = t if c == 1.0 else c * t
            total = term if total is None else total + term
    return total


def _oracle_grads(state, cfg, x):
    """{composition: {key: grad}} from ONE fp32 oracle forward."""
    live = O.live_params(state, cfg)
    P = {k: (v.detach().clone().requires_grad_(True) if k in live else v.detach()) for k, v in state.items()}
    Lo = O.losses(cfg, x, O.forward(P, cfg, x))
    keys = list(live)
    out = {}
    for name, coef in COMPS.items():
        g = torch.autograd.grad(_compose(coef, Lo["train"], Lo["extrap"], Lo["recons"]), [P[k] for k in keys],
                                retain_graph=True, allow_unused=True)
        out[name] = {k: gi for k, gi in zip(keys, g) if gi is not None}
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(oracle grads per composition, envelope bars per composition and key),
    computed once per fixture and only read afterwards."""
    torch.set_num_threads(8)
    z = load_golden(name)
    cfg, _ = O.cfg_from_golden(z)
    state = golden_weights(z)
    x = O.input_from_u8(z["input_u8"])
    ref = _oracle_grads(state, cfg, x)
    worst = {c: dict.fromkeys(g, 0.0) for c, g in ref.items()}
    for seed in range(MEMBERS):
        mem = _oracle_grads(_ulp_perturbed(state, seed), cfg, x)
        for c, g in ref.items():
            assert set(mem[c]) == set(g)
            for k in g:
                worst[c][k] = max(worst[c][k], rel_err(mem[c][k], g[k]))
    bars = {c: {k: max(ENVELOPE_K * v, RT) for k, v in w.items()} for c, w in worst.items()}
    return ref, bars


def _x(name):
    return O.input_from_u8(load_golden(name)["input_u8"]).to(DEV)


def _backward(m, x, comp):
    m.output = m(x)
    train, (_, extrap, recons) = m.compute_loss()
    _compose(COMPS[comp], train, extrap, recons).backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


@functools.lru_cache(maxsize=None)
def _fresh(name, comp):
    """A fresh model's gradients under one composition (default settings)."""
    return _backward(_model(load_golden(name), DEV), _x(name), comp)


def _alive(name, comp, grads):
    """The dead-value guard on reference gradients."""
    for k, g in grads.items():
        if k.startswith("var_net_"):
            assert float(g.abs().max()) > 0, f"{name} {comp}: reference gradient of {k} is identically zero"
    if COMPS[comp][0] != 0.0 or COMPS[comp][1] != 0.0:
        assert float(grads[PHYS[name]].abs().max()) > 0, f"{name} {comp}: {PHYS[name]} has a zero reference gradient"


@pytest.mark.parametrize("comp", list(COMPS))
@pytest.mark.parametrize("name", FIXTURES)
def test_composition_matches_oracle(name, comp):
    ref, bars = _oracle(name)
    ref, bars = ref[comp], bars[comp]
    _alive(name, comp, ref)
    got = _fresh(name, comp)
    assert set(got) == set(ref), set(got) ^ set(ref)
    if comp == "recons":
        assert not any(k.startswith(("velocity_encoder.", "rollout_cell.")) for k in got)
    errs = {k: rel_err(got[k], ref[k]) for k in ref}
    k_, e_ = max(errs.items(), key=lambda kv: kv[1] / bars[kv[0]])
    print(f"{name} {comp}: worst vs bar {k_} {e_:.2e} (bar {bars[k_]:.2e})")
    for k, g in ref.items():
        if float(g.abs().max()) == 0:
            assert float(got[k].abs().max()) == 0, f"{k}: oracle gradient is zero, device's is not"
    over = {k: (e, bars[k]) for k, e in errs.items() if not e <= bars[k]}
    assert not over, over


@pytest.mark.parametrize("comp", list(COMPS))
@pytest.mark.parametrize("name", FIXTURES)
def test_composition_inkernel_equals_arrays(name, comp, monkeypatch):
    want = _fresh(name, comp)
    _alive(name, comp, want)
    monkeypatch.setenv("PAIG_LOSSW_INKERNEL", "0")
    got = _backward(_model(load_golden(name), DEV), _x(name), comp)
    assert set(got) == set(want)
    diff = [k for k in want if not torch.equal(got[k], want[k])]
    assert not diff, diff


@pytest.mark.parametrize("first,second", [("train", "train+0.5extrap"), ("train+0.5extrap", "train")])
@pytest.mark.parametrize("name", FIXTURES)
def test_compositions_in_sequence(name, first, second):
    """A backward with (without) the extrapolation loss, zero_grad, a new
    forward, then one without (with) it: nothing of the first may survive --
    neither the live-steps mark that skips the extrapolation frames, nor its
    adjoints."""
    want = _fresh(name, second)
    _alive(name, second, want)
    m = _model(load_golden(name), DEV)
    x = _x(name)
    _backward(m, x, first)
    m.zero_grad(set_to_none=True)
    got = _backward(m, x, second)
    assert set(got) == set(want)
    worst, key = worst_err({k: (got[k], want[k]) for k in want})
    print(f"{name} {first} then {second}: worst {worst:.2e} at {key}")
    assert worst <= 1e-5, (worst, key)


@pytest.mark.parametrize("name", FIXTURES)
def test_compute_loss_twice_on_one_forward(name):
    """Two compute_loss() calls on ONE forward, terms of both in the loss:
    the forward's backward receives two sets of adjoints (the materialised-
    weights path) and must give the gradients of train + 0.5 extrap."""
    want = _fresh(name, "train+0.5extrap")
    _alive(name, "train+0.5extrap", want)
    m = _model(load_golden(name), DEV)
    m.output = m(_x(name))
    train_a, _ = m.compute_loss()
    _, (_, extrap_b, _) = m.compute_loss()
    (train_a + 0.5 * extrap_b).backward()
    torch.cuda.synchronize()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    worst, key = worst_err({k: (got[k], want[k]) for k in want})
    print(f"{name} compute_loss twice: worst {worst:.2e} at {key}")
    assert worst <= 1e-5, (worst, key)


@pytest.mark.parametrize("name", FIXTURES)
def test_two_models_one_backward(name):
    """m1(x0), m2(x1), both compute_loss(), then ONE backward of
    train1 + 3 train2 + 0.5 extrap2: each model's gradients are those of its
    own loss alone (the models share shapes, so anything keyed by shape)."""
    z = load_golden(name)
    x0 = _x(name)
    x1 = x0[:, :, [1, 2, 0]].flip(0).contiguous()   # other frames: channels rotated, batch reversed

    def alone(x, coef):
        m = _model(z, DEV)
        m.output = m(x)
        train, (_, extrap, recons) = m.compute_loss()
        _compose(coef, train, extrap, recons).backward()
        torch.cuda.synchronize()
        return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    want1, want2 = alone(x0, (1.0, 0.0, 0.0)), alone(x1, (3.0, 0.5, 0.0))
    _alive(name, "train", want1)
    _alive(name, "train+0.5extrap", want2)
    # the two losses' gradients differ, so a mix-up shows
    assert rel_err(want2["var_net_content.l2.weight"], want1["var_net_content.l2.weight"]) > 1e-2
    m1, m2 = _model(z, DEV), _model(z, DEV)
    m1.output, m2.output = m1(x0), m2(x1)
    t1, _ = m1.compute_loss()
    t2, (_, e2, _) = m2.compute_loss()
    (t1 + 3 * t2 + 0.5 * e2).backward()
    torch.cuda.synchronize()
    for m, want, tag in ((m1, want1, "m1"), (m2, want2, "m2")):
        got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
        assert set(got) == set(want), tag
        worst, key = worst_err({k: (got[k], want[k]) for k in want})
        print(f"{name} {tag}: worst {worst:.2e} at {key}")
        assert worst <= 1e-5, (tag, worst, key)
