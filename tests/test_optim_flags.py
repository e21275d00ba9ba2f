"""CPU checks of the gradient-norm options' plumbing: the runner's additive
flags and FlatParams.group_of over every live parameter name of every task."""
import os
import sys

import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(REPO, "runners"))

from test_runner import REFERENCE_FLAGS  # noqa: E402


def test_parser_has_the_optimizer_flags():
    import torch_run_physics as R
    ns = R.build_parser().parse_args([])
    assert ns.clip_grad_norm == 0.0 and ns.physics_lr_mult == 1.0 and ns.log_grad_norms is False
    for k, v in REFERENCE_FLAGS.items():
        assert getattr(ns, k) == v, k
    ns = R.build_parser().parse_args(["--clip_grad_norm", "2.5", "--physics_lr_mult", "10", "--log_grad_norms"])
    assert ns.clip_grad_norm == 2.5 and ns.physics_lr_mult == 10.0 and ns.log_grad_norms is True


def test_build_optimizer_keeps_the_reference_signature():
    import inspect
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    ps = list(inspect.signature(PhysicsNet.build_optimizer).parameters.values())
    assert [p.name for p in ps[:4]] == ["self", "base_lr", "optimizer", "anneal_lr"]
    assert (ps[2].default, ps[3].default) == ("rmsprop", True)
    assert {p.name: p.default for p in ps[4:]} == {"max_grad_norm": None, "physics_lr_mult": None, "grad_norms": None}


@pytest.mark.parametrize("task", ["bouncing_balls", "spring_color", "spring_color_half", "3bp_color",
                                  "mnist_spring_color"])
def test_group_of_covers_every_live_name(task):
    import torch_run_physics as R
    from paig_reproduction_amd.flat import GROUPS, FlatParams, _GROUP_PREFIXES
    from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
    _, _, cell, seq_len, _, ins, pred, size = R.TASKS[task]
    m = PhysicsNet(task, 100, 1, cell, seq_len, ins, pred, 3.0, False, True, size, "conv_encoder", "conv_st_decoder",
                   device=torch.device("cpu"))
    names = m._live_names()
    assert len(names) > 20
    seen = set()
    for n in names:
        g = FlatParams.group_of(n)
        assert g in GROUPS
        # exactly one group: the first matching prefix decides, and only a U-Net
        # name matches two prefixes (its own and the encoder's)
        hits = {grp for prefix, grp in _GROUP_PREFIXES if n.startswith(prefix)}
        assert hits == {g} or hits == {"unet", "localiser"} and g == "unet", (n, hits)
        seen.add(g)
    want = {"unet", "localiser", "velocity", "decoder"} | ({"physics"} if cell != "bouncing_ode_cell" else set())
    assert seen == want, (task, seen)
    with pytest.raises(KeyError):
        FlatParams.group_of("not_a_parameter.weight")
