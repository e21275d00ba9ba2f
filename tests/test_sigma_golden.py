"""Pin the sigma-patched oracle (tests/sigma_ref.py) to the reference run with
``log_sig = 2.0`` (tests/golden/gen_golden_sigma.py), at test_oracle_golden.py's
own bars, and to the unpatched oracle at sigma = 1 bit for bit.  Also the
runner's ``--sigma`` option."""
import os
import types

import numpy as np
import torch

from helpers import GOLDEN_DIR, golden_weights, assert_close, grad_checks
from oracle import physics_oracle as O
import sigma_ref as SR

ORACLE_RTOL = 2e-6    # test_oracle_golden.py's bars
GRAD_RTOL = 2e-5


def load_sigma_golden():
    return np.load(os.path.join(GOLDEN_DIR, "sigma", "golden_spring_s12_sigma2.npz"), allow_pickle=False)


def test_fixture_is_not_a_sigma1_golden():
    """helpers.GOLDEN (the sigma = 1 tests' list) must not contain it."""
    from helpers import GOLDEN
    assert not any("sigma" in n for n in GOLDEN)
    assert float(load_sigma_golden()["log_sig"]) == 2.0


def test_patched_oracle_matches_reference_sigma2():
    torch.set_num_threads(4)
    z = load_sigma_golden()
    cfg, B = O.cfg_from_golden(z)
    state = golden_weights(z)
    x = O.input_from_u8(z["input_u8"])
    with SR.patched_oracle(float(z["log_sig"])):
        out, L, grads = O.train_step(state, cfg, x)
    assert O.st_decoder.__module__ == O.__name__   # restored
    for k in ("enc_pos", "enc_masks", "recons_out"):
        assert_close(out[k], z[k], ORACLE_RTOL, k)
    for k in ("output_seq", "pos_vel_seq"):
        assert_close(out[k], z[k], 1e-5, k)
    assert_close(L["recons"], z["loss_recons"], ORACLE_RTOL, "recons")
    assert_close(L["extrap"], z["loss_extrap"], ORACLE_RTOL, "extrap")
    assert_close(L["pred"], z["loss_pred_true"], ORACLE_RTOL, "pred")
    assert_close(L["train"], z["loss_train"], ORACLE_RTOL, "train")
    grad_checks(z, grads, GRAD_RTOL)
    assert sorted(grads) == sorted(str(k) for k in z["grad_keys"])
    # sigma = 2 is not sigma = 1: the fixture differs from the plain one
    z1 = np.load(os.path.join(GOLDEN_DIR, "golden_spring_s12.npz"), allow_pickle=False)
    assert np.abs(z["recons_out"] - z1["recons_out"]).max() > 1e-2


def test_helper_equals_oracle_at_sigma1():
    g = torch.Generator().manual_seed(5)
    for K, H in ((2, 32), (3, 36)):
        h = H // 2
        cfg = types.SimpleNamespace(n_objs=K, tmpl=h, size=H)
        joint = torch.randn(K, 6, h, h, generator=g)
        bg = torch.rand(1, 3, H, H, generator=g)
        pos = (torch.rand(7, 2 * K, generator=g) * 1.5 - 0.25) * H
        sigma = SR.sigma_of(1.0)
        assert torch.equal(SR.st_decoder_sigma(cfg, joint, bg, pos, sigma), O.st_decoder(cfg, joint, bg, pos))
        c, m = SR.st_decoder_parts_sigma(cfg, joint, bg, pos, sigma)
        rc, rm = O.st_decoder_parts(cfg, joint, bg, pos)
        for a, b in zip(list(c) + list(m), list(rc) + list(rm)):
            assert torch.equal(a, b)


def test_reference_sigma_expression():
    """np.exp(np.log(.)) as the reference forms sigma: exact for 0.5, 1, 1.5
    and 2; for other values (0.7) whatever the platform's exp / log give, to
    an ulp -- which is why the model evaluates the same expression."""
    for v in (0.5, 1.0, 1.5, 2.0):
        assert SR.sigma_of(v) == v
    assert abs(SR.sigma_of(0.7) - 0.7) <= 2.3e-16


def test_runner_sigma_option():
    import importlib.util
    path = os.path.join(os.path.dirname(GOLDEN_DIR), "..", "runners", "torch_run_physics.py")
    spec = importlib.util.spec_from_file_location("torch_run_physics_sigma", os.path.abspath(path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    assert p.parse_args([]).sigma == 1.0
    assert p.parse_args(["--sigma", "2.0"]).sigma == 2.0
