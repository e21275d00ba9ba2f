"""The engine's host-side records (no GPU, no library call): the typed step
state, the live-steps decision of the rollout decoder backward, and the A/B
switch record."""
import pytest

from paig_reproduction_amd._lib import PaigError
from paig_reproduction_amd.engine import LossAdjoints, StepState, Switches, live_steps, read_switches


def test_state_rejects_undeclared_attribute():
    S = StepState()
    with pytest.raises(AttributeError):
        S.dense_tial = True
    with pytest.raises(AttributeError):
        S.acts = {}


def test_state_defaults():
    S = StepState()
    assert S.extra_slabs == [] and S.extra_slabs is not StepState().extra_slabs
    assert S.dense_tail is False and S.consumed is False
    assert S.need_saved is True
    assert S.unet_ws is None and S.probe_cb is None and S.vel0 is None


def test_state_release_and_freshness():
    S = StepState()
    S.check_fresh()
    S.unet_ws = object()
    S.check_fresh()
    S.release()
    assert S.unet_ws is None
    for _ in range(2):   # keeps raising
        with pytest.raises(PaigError, match=r"a second backward through one forward \(retain_graph=True\) is not "
                                            r"supported: the forward's saved state \(its U-Net workspace\) was "
                                            r"released by the first backward"):
            S.check_fresh()


T = object()   # stands for a 0-d adjoint tensor


def _adj(de=None, pred=6):
    return LossAdjoints(dt=T, de=de, dr=T, ae=3.0, B=4, Te=10, R=46, pred=pred)


def test_live_steps():
    train = (True, _adj())
    assert live_steps(None, None, [train]) == 6                   # train-only adjoints: pred
    assert live_steps(None, None, [(True, _adj(de=T))]) == 0      # an extrapolation adjoint
    assert live_steps(None, None, [train, (True, _adj(de=T))]) == 0
    assert live_steps(object(), None, [train]) == 0               # a dense d_out
    assert live_steps(None, object(), [train]) == 0               # a gradient on the public rollout SSE
    assert live_steps(None, None, []) == 0                        # no entries
    assert live_steps(None, None, [train, (False, _adj())]) == 6  # two train-only entries
    assert live_steps(None, None, [(False, _adj(pred=3))]) == 3


def test_loss_adjoints_fields():
    assert LossAdjoints._fields == ("dt", "de", "dr", "ae", "B", "Te", "R", "pred")
    a = _adj(pred=5)
    assert a[7] == a.pred == 5 and a[1] is a.de is None


SWITCH_ENV = {"fuse_head": "PAIG_FUSE_HEAD", "dense_tail": "PAIG_DENSE_TAIL", "fuse_vfn": "PAIG_FUSE_VFN",
              "merge_roll": "PAIG_MERGE_ROLL", "fused_bwd": "PAIG_FUSED_BWD", "upt": "PAIG_UPT",
              "pool_fold": "PAIG_POOL_FOLD", "wprep_merge": "PAIG_WPREP_MERGE", "fuse_vel": "PAIG_FUSE_VEL",
              "fuse_vfn2": "PAIG_FUSE_VFN2", "gemm_epi_merge": "PAIG_GEMM_EPI_MERGE"}


@pytest.fixture
def clean_env(monkeypatch):
    for name in list(SWITCH_ENV.values()) + ["PAIG_SCHED"]:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_switches_default_on(clean_env):
    sw = read_switches()
    assert Switches._fields == tuple(SWITCH_ENV)
    assert all(sw), sw
    with pytest.raises(AttributeError):   # frozen
        sw.fuse_vel = False


@pytest.mark.parametrize("field", list(SWITCH_ENV))
def test_switch_off_turns_exactly_that_field_off(clean_env, field):
    clean_env.setenv(SWITCH_ENV[field], "0")
    sw = read_switches()
    assert [f for f in Switches._fields if not getattr(sw, f)] == [field]
    clean_env.setenv(SWITCH_ENV[field], "1")
    assert all(read_switches())
    clean_env.setenv(SWITCH_ENV[field], "")   # only "0" turns a switch off
    assert all(read_switches())


def test_retired_schedule_switch_changes_nothing(clean_env):
    clean_env.setenv("PAIG_SCHED", "0")
    assert read_switches() == Switches(*[True] * len(Switches._fields))
