"""CPU checks of the learnable attention-window scale (no GPU needed):
the autograd yardstick tests/sigma_grad_ref.py restates tests/sigma_ref.py
exactly at constant sigma, the parametrisation's constructor rules, the
gradient-norm group of the new parameter, and the runner's flag."""
import types

import numpy as np
import pytest
import torch

import sigma_grad_ref as SG
import sigma_ref as SR


def _cfg(K, H):
    return types.SimpleNamespace(n_objs=K, tmpl=H // 2, size=H)


@pytest.mark.parametrize("K,H", [(2, 32), (3, 36), (2, 16)])
@pytest.mark.parametrize("sigma", [0.5, 0.7, 1.0, 1.5, 2.0])
def test_helper_forward_equals_sigma_ref(K, H, sigma):
    g = torch.Generator().manual_seed(K * 100 + H)
    h = H // 2
    joint = torch.cat([torch.randn(K, 1, h, h, generator=g).repeat(1, 3, 1, 1) + 5,
                       torch.sigmoid(torch.randn(K, 3, h, h, generator=g))], 1)
    bg = torch.sigmoid(torch.randn(1, 3, H, H, generator=g))
    pos = (torch.rand(6, 2 * K, generator=g) * 1.5 - 0.25) * H
    s = SR.sigma_of(sigma)
    want = SR.st_decoder_sigma(_cfg(K, H), joint, bg, pos, s)
    for st in (torch.tensor(s, dtype=torch.float64), torch.tensor([s], dtype=torch.float64),
               torch.full((6,), s, dtype=torch.float64)):
        assert torch.equal(SG.st_decoder_sigma(_cfg(K, H), joint, bg, pos, st), want)
    wc, wm = SR.st_decoder_parts_sigma(_cfg(K, H), joint, bg, pos, s)
    gc, gm = SG.st_decoder_parts_sigma(_cfg(K, H), joint, bg, pos, torch.tensor(s, dtype=torch.float64))
    for a, b in zip(list(gc) + list(gm), list(wc) + list(wm)):
        assert torch.equal(a, b)


def test_sigma_from_u_is_one_at_zero_and_inside_the_range():
    assert float(SG.sigma_from_u(torch.zeros(()))) == 1.0
    for u in (-30.0, -3.0, 3.0, 30.0):
        assert 0.5 <= float(SG.sigma_from_u(torch.tensor(u))) <= 2.0


def _net(**kw):
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    torch.manual_seed(0)
    return PhysicsNet("spring_color", 100, 1, "spring_ode_cell", 12, 3, 5, 3.0, False, True, 32 * 32, "conv_encoder",
                      "conv_st_decoder", **kw)


def test_parametrisation_constructor_rules():
    off = _net()
    assert len(off.state_dict()) == 93
    assert "decoder_sigma_u" not in dict(off.named_parameters())
    assert "decoder_sigma_u" not in off._flat.names and not hasattr(off, "decoder_sigma_u")
    off.log_sig = 1.5   # the fixed mode's attribute stays assignable
    on = _net(sigma=1.5, learn_sigma=True)
    assert len(on.state_dict()) == 94
    u = on.decoder_sigma_u
    assert u.dtype == torch.float32 and u.dim() == 0
    assert float(u.detach()) == float(np.float32(np.arctanh(np.log(1.5) / np.log(2.0))))
    assert abs(on.decoder_sigma() - 1.5) < 1e-6
    assert float(_net(learn_sigma=True).decoder_sigma_u.detach()) == 0.0 and _net(learn_sigma=True).decoder_sigma() == 1.0
    # appended to the late part of the fp32 names: every other name where it was
    assert on._flat.names[:-3] == off._flat.names[:-2] and on._flat.names[-3] == "decoder_sigma_u"
    assert on._flat.names[-2:] == off._flat.names[-2:] == ["rollout_cell.k", "rollout_cell.equil"]
    with pytest.raises(AttributeError, match="decoder_sigma_u"):
        on.log_sig = 1.0
    for bad in (2.0, 0.5, 2.5, 0.1):
        with pytest.raises(ValueError, match="sigma"):
            _net(sigma=bad, learn_sigma=True)


def test_gradient_norm_group_is_decoder():
    from paig_reproduction_amd.flat import FlatParams
    assert FlatParams.group_of("decoder_sigma_u") == "decoder"
    assert FlatParams.group_of("var_net_template.l1.weight") == "decoder"
    assert FlatParams.group_of("rollout_cell.k") == "physics"


def test_runner_flag():
    from runners.torch_run_physics import build_parser
    p = build_parser()
    base = ["--task", "spring_color"]
    assert p.parse_args(base).learn_sigma is False
    a = p.parse_args(base + ["--learn_sigma", "--sigma", "1.5"])
    assert a.learn_sigma is True and a.sigma == 1.5
