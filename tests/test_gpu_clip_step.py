"""FlatOptimizer's gradient-norm clipping, physics learning-rate multiplier
and per-group gradient norms on the spring_s12 fixture, against
torch.nn.utils.clip_grad_norm_ + torch.optim on the same gradients (the
pattern of test_gpu_training.py::test_optimizer_matches_torch).

Parameter bar: the project's envelope rule (tests/envelope.py).  The references
run once in float64 (the truth) and once in fp32 (the honest fp32 run: the fp32
parameters and torch's fp32 clip; the float64 physics parameters stay float64
as in the model); a parameter may sit no further from the truth than
max(ENVELOPE_K * e32, ENVELOPE_FLOOR), e32 the fp32 run's own distance.

FlatOptimizer leaves p.grad unclipped, so every step clips fresh gradients: the
torch references get the unclipped gradients back before each step.
"""
import logging
import math

import pytest
import torch

from envelope import ENVELOPE_FLOOR, ENVELOPE_K
from helpers import load_golden, rel_err
from test_gpu_training import _model, _x

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LR = 1e-3
KINDS = ["rmsprop", "adam", "sgd", "momentum"]
OFF = dict(max_grad_norm=0.0, physics_lr_mult=1.0, grad_norms=False)
EPS = 2.0 ** -52


def _backward(m, x, seed=None):
    m.output = m(x)
    tl, _ = m.compute_loss()
    m.optimizer.zero_grad(set_to_none=True)
    if seed is None:
        tl.backward()
    else:
        tl.backward(seed(tl))
    torch.cuda.synchronize()
    return tl


def _norm64(grads):
    return math.sqrt(sum(float((g.detach().double().cpu() ** 2).sum()) for g in grads))


@pytest.fixture(scope="module")
def ctx():
    """One model, one real backward: the parameters are restored and the
    optimizer rebuilt per run; the gradients stay in the flat buffers."""
    z = load_golden("spring_s12")
    m = _model(z, DEV)
    m.build_optimizer(LR, "rmsprop", True, **OFF)
    _backward(m, _x(z["input_u8"], DEV))
    named = {k: p for k, p in m.named_parameters() if p.grad is not None}
    c = {"m": m, "named": named, "p32": m._flat.p32.clone(), "p64": m._flat.p64.clone(),
         "p0": {k: p.detach().cpu().clone() for k, p in named.items()},
         "g0": {k: p.grad.detach().cpu().clone() for k, p in named.items()}, "refs": {}}
    c["norm"] = _norm64(c["g0"].values())
    assert c["norm"] > 0 and any(p.dtype == torch.float64 for p in named.values())
    return c


def _hip(ctx, kind, steps=3, **opt):
    m = ctx["m"]
    with torch.no_grad():
        m._flat.p32.copy_(ctx["p32"])
        m._flat.p64.copy_(ctx["p64"])
    m.build_optimizer(LR, kind, True, **{**OFF, **opt})
    for _ in range(steps):
        m.optimizer.step()
    torch.cuda.synchronize()
    return {k: p.detach().cpu().clone() for k, p in ctx["named"].items()}


def _torch(ctx, kind, max_norm, mult, f64, steps=3):
    """clip_grad_norm_ + torch.optim from the same parameters and gradients;
    the physics parameters in a group of their own with lr * mult."""
    key = (kind, max_norm, mult, f64)
    if key in ctx["refs"]:
        return ctx["refs"][key]
    # always a copy: the references step and clip in place
    cast = (lambda t: t.to(torch.float64, copy=True)) if f64 else (lambda t: t.clone())
    ref = {k: torch.nn.Parameter(cast(v)) for k, v in ctx["p0"].items()}
    phys = [k for k in ref if k.startswith("rollout_cell.")]
    groups = [{"params": [ref[k] for k in ref if k not in phys]},
              {"params": [ref[k] for k in phys], "lr": LR * mult}]
    opt = {"adam": lambda g: torch.optim.Adam(g, lr=LR), "rmsprop": lambda g: torch.optim.RMSprop(g, lr=LR),
           "momentum": lambda g: torch.optim.SGD(g, momentum=0.9, lr=LR), "sgd": lambda g: torch.optim.SGD(g, lr=LR)}[
        kind](groups)
    for _ in range(steps):
        for k, p in ref.items():
            p.grad = cast(ctx["g0"][k])
        if max_norm:
            torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm)
        opt.step()
    out = {k: p.detach().clone() for k, p in ref.items()}
    ctx["refs"][key] = out
    return out


def _assert_envelope(ctx, got, kind, max_norm, mult, what):
    r64, r32 = _torch(ctx, kind, max_norm, mult, True), _torch(ctx, kind, max_norm, mult, False)
    for k in got:
        e32 = rel_err(r32[k].double(), r64[k])
        e = rel_err(got[k].double(), r64[k])
        bar = max(ENVELOPE_K * e32, ENVELOPE_FLOOR)
        print(what, kind, k, f"hip {e:.2e} fp32 {e32:.2e} bar {bar:.2e}")
        assert e <= bar, (what, kind, k, e, e32)


def _bits_equal(a, b, keys=None):
    return [k for k in (keys or a) if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("kind", KINDS)
def test_clip_matches_torch(ctx, kind):
    n = ctx["norm"]
    off = _hip(ctx, kind)
    active = _hip(ctx, kind, max_grad_norm=0.5 * n)
    coef = float(ctx["m"].optimizer._gn[1][1])
    assert abs(coef - 0.5 * n / (n + 1e-6)) <= 1e-12
    inactive = _hip(ctx, kind, max_grad_norm=2.0 * n)
    assert float(ctx["m"].optimizer._gn[1][1]) == 1.0
    _assert_envelope(ctx, active, kind, 0.5 * n, 1.0, "clip active")
    _assert_envelope(ctx, inactive, kind, 2.0 * n, 1.0, "clip inactive")
    assert _bits_equal(inactive, off) == [], "an inactive clip changed parameter bits"
    assert _bits_equal(active, off) != []
    # p.grad keeps the unclipped gradient (unlike torch's in-place clip)
    assert _bits_equal({k: p.grad.detach().cpu() for k, p in ctx["named"].items()}, ctx["g0"]) == []


@pytest.mark.parametrize("kind", KINDS)
def test_physics_lr_mult(ctx, kind):
    base = _hip(ctx, kind)
    got = _hip(ctx, kind, physics_lr_mult=10.0)
    _assert_envelope(ctx, got, kind, 0.0, 10.0, "physics_lr_mult")
    f32 = [k for k, v in got.items() if v.dtype == torch.float32]
    f64 = [k for k, v in got.items() if v.dtype == torch.float64]
    assert _bits_equal(got, base, f32) == []
    assert f64 and _bits_equal(got, base, f64) == f64
    # with clipping too: the clipped kernels take the same two learning rates
    n = ctx["norm"]
    both = _hip(ctx, kind, physics_lr_mult=10.0, max_grad_norm=0.5 * n)
    _assert_envelope(ctx, both, kind, 0.5 * n, 10.0, "physics_lr_mult + clip")


@pytest.mark.parametrize("kind", KINDS)
def test_defaults_change_nothing(ctx, kind):
    """All three features off: paig_grad_norm is never called and the
    parameters are those of a FlatOptimizer built the old way."""
    from paig_reproduction_amd._lib import lib
    from paig_reproduction_amd.flat import FlatOptimizer
    L = lib()
    real, calls = L.fns["paig_grad_norm"], []

    def counted(*a):
        calls.append(1)
        return real(*a)

    L.fns["paig_grad_norm"] = counted
    try:
        new = _hip(ctx, kind)
        m = ctx["m"]
        with torch.no_grad():
            m._flat.p32.copy_(ctx["p32"])
            m._flat.p64.copy_(ctx["p64"])
        m.optimizer = (FlatOptimizer(m, "sgd", LR, momentum=0.9) if kind == "momentum" else
                       FlatOptimizer(m, "sgd" if kind == "sgd" else kind, LR))
        for _ in range(3):
            m.optimizer.step()
        torch.cuda.synchronize()
        old = {k: p.detach().cpu().clone() for k, p in ctx["named"].items()}
        assert calls == []
        _hip(ctx, kind, steps=1, grad_norms=True)
        assert calls == [1]   # the counter does see the launch when a feature is on
    finally:
        L.fns["paig_grad_norm"] = real
    assert _bits_equal(new, old) == []
    assert _bits_equal(new, ctx["p0"]) != []


def test_state_dict_carries_the_options(ctx):
    m = ctx["m"]
    m.build_optimizer(LR, "adam", True, max_grad_norm=2.5, physics_lr_mult=4.0, grad_norms=True)
    sd = m.optimizer.state_dict()
    assert {k: sd["param_groups"][0][k] for k in OFF} == dict(max_grad_norm=2.5, physics_lr_mult=4.0, grad_norms=True)
    m.build_optimizer(LR, "adam", True, **OFF)
    m.optimizer.load_state_dict(sd)
    assert {k: m.optimizer.param_groups[0][k] for k in OFF} == dict(max_grad_norm=2.5, physics_lr_mult=4.0,
                                                                     grad_norms=True)


@pytest.mark.parametrize("kind", ["rmsprop", "adam", "momentum"])
def test_per_parameter_path_clips_over_params_with_grad(kind):
    """The scenario of test_optimizer_skips_params_without_grad: after a
    full step and zero_grad, a standalone encoder backward.  The norm covers
    the encoder's gradients alone (the other parameters' slots still hold the
    previous step's values), the encoder moves as clip_grad_norm_ + torch.optim
    move it, nothing else moves."""
    z = load_golden("spring_s12")
    m = _model(z, DEV)
    m.build_optimizer(LR, kind, True, **{**OFF, "grad_norms": True})
    x = _x(z["input_u8"], DEV)
    make = {"adam": lambda ps: torch.optim.Adam(ps, lr=LR), "rmsprop": lambda ps: torch.optim.RMSprop(ps, lr=LR),
            "momentum": lambda ps: torch.optim.SGD(ps, momentum=0.9, lr=LR)}[kind]
    _backward(m, x)
    named = {k: p for k, p in m.named_parameters() if p.grad is not None}
    ref = {k: torch.nn.Parameter(p.detach().clone()) for k, p in named.items()}
    for k, p in ref.items():
        p.grad = named[k].grad.detach().clone()
    topt = make(list(ref.values()))
    topt.step()
    m.optimizer.step()
    full = float(m.optimizer.grad_norms()["total"])
    m.optimizer.zero_grad(set_to_none=True)
    topt.zero_grad(set_to_none=True)
    frames = x[:, :m.input_steps + m.pred_steps].reshape(-1, 3, 32, 32)
    pos, _, _ = m.encoder(frames)
    pos.sum().backward()
    torch.cuda.synchronize()
    enc = [k for k, p in named.items() if p.grad is not None]
    assert enc and all(k.startswith("encoder.") for k in enc) and len(enc) < len(named)
    n_enc = _norm64([named[k].grad for k in enc])
    m.optimizer.param_groups[0]["max_grad_norm"] = 0.5 * n_enc
    for k in enc:
        ref[k].grad = named[k].grad.detach().clone()
    torch.nn.utils.clip_grad_norm_([ref[k] for k in enc], 0.5 * n_enc)
    before = {k: p.detach().clone() for k, p in named.items()}
    topt.step()
    m.optimizer.step()
    torch.cuda.synchronize()
    norms = m.optimizer.grad_norms()
    count = sum(named[k].numel() for k in enc)
    print(kind, "encoder-only norm", float(norms["total"]), n_enc, "full step's", full)
    assert abs(float(norms["total"]) - n_enc) <= count * EPS * n_enc
    assert float(norms["decoder"]) == 0.0 and float(norms["physics"]) == 0.0 and full != float(norms["total"])
    for k, p in named.items():
        if k in enc:
            # the fixed floor of the envelope rule: the fp32 torch run is the reference here
            assert rel_err(p.detach(), ref[k].detach()) <= ENVELOPE_FLOOR, (kind, k)
            assert not torch.equal(p.detach(), before[k])
        else:
            assert torch.equal(p.detach(), before[k]), f"{kind}: {k} moved without a gradient"


def test_graph_and_eager_agree(ctx):
    """5 steps with the optimizer in the graph, 5 with the eager tail, 5 in
    plain eager: parameters and the norm record are bit-identical."""
    from paig_reproduction_amd.graph_step import GraphStep
    z = load_golden("spring_s12")
    x = _x(z["input_u8"], DEV)
    runs = []
    for mode in ("in_graph", "eager_tail", "eager"):
        m = _model(z, DEV)
        m.build_optimizer(LR, "rmsprop", True, max_grad_norm=0.5 * ctx["norm"], physics_lr_mult=1.0, grad_norms=True)
        xbuf = x.clone()
        gs = GraphStep(m, xbuf, 1, graph=mode != "eager", optimizer_in_graph=mode == "in_graph")
        assert gs.opt_in_graph == (mode == "in_graph")
        gs.eager()
        first = float(m.optimizer._gn[1][1])
        print(mode, "first step: coef", first, "norm", float(m.optimizer._gn[1][0]))
        assert first < 1.0                     # the clip is active on the measured gradients
        gs.eager()
        gs.capture()
        for _ in range(3):
            gs()
        gs.finish()
        torch.cuda.synchronize()
        runs.append(({k: p.detach().cpu().clone() for k, p in m.named_parameters()},
                     m.optimizer._gn[1].cpu().clone()))
    for params, stats in runs[1:]:
        assert _bits_equal(params, runs[0][0]) == []
        assert torch.equal(stats.view(torch.int64), runs[0][1].view(torch.int64))


def _spring(live):
    from paig_reproduction_amd.nn.datasets.synth import as_model_input, render_sequences
    z = load_golden("spring_s12")
    if live:
        m = _model(z, DEV)
    else:
        from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
        torch.manual_seed(0)
        m = PhysicsNet("spring_color", 100, 1, "spring_ode_cell", 12, 4, 6, 3.0, False, True, 32 * 32, "conv_encoder",
                       "conv_st_decoder", device=DEV).to(DEV)
    u8 = render_sequences("spring_color", 8, 12, seed=1)
    return m, u8, torch.from_numpy(as_model_input(u8)).to(DEV)


@pytest.mark.parametrize("live", [False, True])
def test_dead_unet_signal(live, tmp_path):
    """At the default init the spring U-Net's gradients are exactly zero (its
    ReLU'd last conv is dead); the per-group norm shows it and train_model
    warns once.  With live-layer weights the group is non-zero and no warning."""
    from paig_reproduction_amd.nn.datasets.iterators import DeviceDataIterator
    m, u8, x = _spring(live)
    m.build_optimizer(LR, "rmsprop", True, **{**OFF, "grad_norms": True})
    _backward(m, x)
    m.optimizer.step()
    norms = {k: float(v) for k, v in m.optimizer.grad_norms().items()}
    print("live" if live else "default init", norms)
    assert set(norms) == {"total", "unet", "localiser", "velocity", "decoder", "physics"}
    assert norms["localiser"] > 0 and norms["total"] > 0
    assert (norms["unet"] > 0) if live else (norms["unet"] == 0.0)
    m.get_data(tuple(DeviceDataIterator(u8, (12, 3, 32, 32), DEV, seed=0) for _ in range(3)))
    m.initialize_graph(str(tmp_path / "run"), False)
    m.extra_test_fns = []
    lines = []

    class Collect(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())

    lg = logging.getLogger("torch")     # the trainer's logger
    handlers, level = list(lg.handlers), lg.level
    lg.addHandler(Collect(level=logging.INFO))
    lg.setLevel(logging.INFO)
    try:
        m.train_model(1, 4, 100, 100, 1, debug=True)     # 8 sequences, batches of 4: two steps, both logged
    finally:
        for h in list(lg.handlers):
            if h not in handlers:
                lg.removeHandler(h)
        lg.setLevel(level)
    train = [s for s in lines if s.startswith("train - iter=")]
    assert len(train) == 2 and all("grad_norm=" in s and "grad_norm/unet=" in s for s in train)
    warned = [s for s in lines if "U-Net gradients are exactly zero" in s]
    assert len(warned) == (0 if live else 1), lines


def test_check_finite_raises_once():
    z = load_golden("spring_s12")
    m = _model(z, DEV)
    m.build_optimizer(LR, "rmsprop", True, **{**OFF, "grad_norms": True})
    _backward(m, _x(z["input_u8"], DEV), seed=lambda tl: torch.full_like(tl, float("inf")))
    m.optimizer.check_finite()        # nothing measured yet
    m.optimizer.step()
    with pytest.raises(FloatingPointError):
        m.optimizer.check_finite()
    m.optimizer.check_finite()        # cleared by the first call
