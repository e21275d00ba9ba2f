"""rollout_ops.RolloutOps on a recording stand-in for the library (no GPU, no
library call): which export every cell's forward and backward reaches from the
engine (B = 100, R = 6) and from the standalone cell module (B = 3, R = 1),
and its argument tuple, element by element, against the tuples the call sites
wrote out by hand before RolloutOps existed; each tuple also against the
export's ctypes signature.  Then the flat gradient buffer's name order of
every cell type, against the lists PhysicsNet._live_names spelt out before."""
import pytest

from paig_reproduction_amd.nn.network import cells
from paig_reproduction_amd.nn.network.physics_models import PhysicsNet
from paig_reproduction_amd.rollout_ops import SPECS, RolloutOps
from test_decoder_ops import ROLL, Dev, RecLib, check_signature

ST = 9         # the stream handle
H = 100        # recurrent_units of the learned cells


class Ws(Dev):
    """Stands for a workspace tensor: its address and its size are read."""

    def __init__(self, addr, numel):
        super().__init__(addr)
        self.n = numel

    def numel(self):
        return self.n


class Lib(RecLib):
    SIZES = {"paig_rollout_bwd_blocks": 7, "paig_rollout_lstm_workspace": 4936, "paig_rollout_in_workspace": 308}


def stand_in(cell_type):
    """A cell of that class name whose operands are addresses 502.. (dt, p0,
    p1) or 510.. (the learned cells' weights, in weights() order)."""
    body = {"spring": dict(dt=Dev(502), k=Dev(503), equil=Dev(504)), "bouncing": dict(dt=Dev(502)),
            "gravity": dict(dt=Dev(502), g=Dev(503), m=Dev(504))}.get(cell_type.split("_")[0].replace("2d", ""))
    if body is None:
        W = tuple(Dev(510 + i) for i in range(len(SPECS[cell_type].names)))
        body = dict(recurrent_units=H, weights=lambda self: W)
    return type(cell_type, (), body)()


def ops(cell_type, B, D, R, half):
    L = Lib()
    return L, RolloutOps(L, stand_in(cell_type), B, D, R, half)


def only_call(L, name, want):
    assert len(L.calls) == 1, L.calls
    got_name, got = L.calls[0]
    assert got_name == name
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w and type(g) is type(w), (name, i, g, w)
    check_signature(name, got)


# ---- the engine: B = 100, R = 6; pos0 500 (row stride 40), vel0 501, pvs 505; adjoints 600.., gradients 801.. ------
# cell type -> (D, half, forward, backward, forward without a workspace or None, flat-gradient slots)
ENGINE = {
    "spring_ode_cell": (
        4, 16.0, ("paig_rollout_fwd", (0, 500, 40, 501, 502, 503, 504, 505, 100, 4, 6, 9)),
        ("paig_rollout_bwd", (0, 505, 600, 601, 502, 503, 504, 602, 603, 604, 801, 802, 0, 100, 4, 6, 9)),
        None, [801, 802]),
    "bouncing_ode_cell": (
        4, 16.0, ("paig_rollout_fwd", (1, 500, 40, 501, 502, None, None, 505, 100, 4, 6, 9)),
        ("paig_rollout_bwd", (1, 505, 600, 601, 502, None, None, 602, 603, 604, None, None, 0, 100, 4, 6, 9)),
        None, []),
    "gravity_ode_cell": (
        6, 18.0, ("paig_rollout_fwd", (2, 500, 40, 501, 502, 503, 504, 505, 100, 6, 6, 9)),
        ("paig_rollout_bwd", (2, 505, 600, 601, 502, 503, 504, 602, 603, 604, 801, None, 0, 100, 6, 6, 9)),
        None, [801]),
    "spring2d_ode_cell": (
        4, 16.0, ("paig_rollout_fwd", (3, 500, 40, 501, 502, 503, 504, 505, 100, 4, 6, 9)),
        ("paig_rollout_bwd", (3, 505, 600, 601, 502, 503, 504, 602, 603, 604, 801, 802, 0, 100, 4, 6, 9)),
        None, [801, 802]),
    "bouncing2d_ode_cell": (
        4, 16.0, ("paig_rollout_fwd", (4, 500, 40, 501, 502, None, None, 505, 100, 4, 6, 9)),
        ("paig_rollout_bwd", (4, 505, 600, 601, 502, None, None, 602, 603, 604, None, None, 0, 100, 4, 6, 9)),
        None, []),
    "lstm_ode_cell": (
        4, 16.0,
        ("paig_rollout_lstm_fwd", (500, 40, 501, 510, 511, 512, 513, 514, 515, 16.0, 505, 700, 4936, 100, 4, 100, 6, 9)),
        ("paig_rollout_lstm_bwd", (600, 601, 510, 511, 514, 16.0, 602, 603, 801, 802, 803, 804, 805, 806, 0, 700, 4936,
                                   100, 4, 100, 6, 9)),
        ("paig_rollout_lstm_fwd", (500, 40, 501, 510, 511, 512, 513, 514, 515, 16.0, 505, None, 0, 100, 4, 100, 6, 9)),
        [801, 802, 803, 804, 805, 806]),
    "interaction_ode_cell": (
        4, 16.0,
        ("paig_rollout_in_fwd", (500, 40, 501, 510, 511, 512, 513, 514, 515, 516, 517, 16.0, 505, 700, 4936, 100, 4, 100,
                                 6, 9)),
        ("paig_rollout_in_bwd", (600, 601, 510, 512, 514, 516, 16.0, 602, 603, 801, 802, 803, 804, 805, 806, 807, 808, 0,
                                 700, 4936, 100, 4, 100, 6, 9)),
        ("paig_rollout_in_fwd", (500, 40, 501, 510, 511, 512, 513, 514, 515, 516, 517, 16.0, 505, None, 0, 100, 4, 100, 6,
                                 9)),
        [801, 802, 803, 804, 805, 806, 807, 808]),
}
# ---- the cell module: B = 3, R = 1; pos 900 (row stride D), vel 901, pvs 902, adjoints 903.., (gk, gq) = 908, 916 ---
# cell type -> (D, half, forward, backward, gradient destinations)
MODULE = {
    "spring_ode_cell": (
        4, None, ("paig_rollout_fwd", (0, 900, 4, 901, 502, 503, 504, 902, 3, 4, 1, 9)),
        ("paig_rollout_bwd", (0, 902, 903, 904, 502, 503, 504, 905, 906, 907, 908, 916, 0, 3, 4, 1, 9)), [908, 916]),
    "bouncing_ode_cell": (
        4, None, ("paig_rollout_fwd", (1, 900, 4, 901, 502, None, None, 902, 3, 4, 1, 9)),
        ("paig_rollout_bwd", (1, 902, 903, 904, 502, None, None, 905, 906, 907, 908, 916, 0, 3, 4, 1, 9)), [908, 916]),
    "gravity_ode_cell": (
        6, None, ("paig_rollout_fwd", (2, 900, 6, 901, 502, 503, 504, 902, 3, 6, 1, 9)),
        ("paig_rollout_bwd", (2, 902, 903, 904, 502, 503, 504, 905, 906, 907, 908, 916, 0, 3, 6, 1, 9)), [908, 916]),
    "spring2d_ode_cell": (
        4, None, ("paig_rollout_fwd", (3, 900, 4, 901, 502, 503, 504, 902, 3, 4, 1, 9)),
        ("paig_rollout_bwd", (3, 902, 903, 904, 502, 503, 504, 905, 906, 907, 908, 916, 0, 3, 4, 1, 9)), [908, 916]),
    "bouncing2d_ode_cell": (
        4, None, ("paig_rollout_fwd", (4, 900, 4, 901, 502, None, None, 902, 3, 4, 1, 9)),
        ("paig_rollout_bwd", (4, 902, 903, 904, 502, None, None, 905, 906, 907, 908, 916, 0, 3, 4, 1, 9)), [908, 916]),
    "lstm_ode_cell": (
        4, 16.0, ("paig_rollout_lstm_fwd", (900, 4, 901, 510, 511, 512, 513, 514, 515, 16.0, 902, 950, 308, 3, 4, 100, 1, 9)),
        ("paig_rollout_lstm_bwd", (None, 904, 510, 511, 514, 16.0, 905, 906, 961, 962, 963, 964, 965, 966, 0, 950, 308, 3,
                                   4, 100, 1, 9)), [961, 962, 963, 964, 965, 966]),
    "interaction_ode_cell": (
        4, 16.0,
        ("paig_rollout_in_fwd", (900, 4, 901, 510, 511, 512, 513, 514, 515, 516, 517, 16.0, 902, 950, 308, 3, 4, 100, 1, 9)),
        ("paig_rollout_in_bwd", (None, 904, 510, 512, 514, 516, 16.0, 905, 906, 961, 962, 963, 964, 965, 966, 967, 968, 0,
                                 950, 308, 3, 4, 100, 1, 9)), [961, 962, 963, 964, 965, 966, 967, 968]),
}
CELL_TYPES = list(SPECS)


def test_the_tables_cover_the_seven_cells():
    assert CELL_TYPES == ["spring_ode_cell", "bouncing_ode_cell", "gravity_ode_cell", "spring2d_ode_cell",
                          "bouncing2d_ode_cell", "lstm_ode_cell", "interaction_ode_cell"]
    assert list(ENGINE) == CELL_TYPES and list(MODULE) == CELL_TYPES


@pytest.mark.parametrize("cell_type", CELL_TYPES)
def test_engine_forward(cell_type):
    D, half, (name, want), _, no_ws, _ = ENGINE[cell_type]
    L, r = ops(cell_type, 100, D, 6, half)
    r.fwd(500, 40, 501, 505, Ws(700, 1234) if r.learned else None, ST)
    only_call(L, name, want)
    if no_ws is not None:   # an absent workspace: (NULL, 0 bytes)
        L, r = ops(cell_type, 100, D, 6, half)
        r.fwd(500, 40, 501, 505, None, ST)
        only_call(L, *no_ws)
    assert r.learned == (no_ws is not None)


@pytest.mark.parametrize("cell_type", CELL_TYPES)
def test_engine_backward(cell_type):
    D, half, _, (name, want), _, grads = ENGINE[cell_type]
    L, r = ops(cell_type, 100, D, 6, half)
    r.bwd(505, 600, 601, 602, 603, grads, 604, Ws(700, 1234) if r.learned else None, 0, ST)
    only_call(L, name, want)


@pytest.mark.parametrize("cell_type", CELL_TYPES)
def test_module_forward_and_backward(cell_type):
    D, half, (fname, fwant), (bname, bwant), grads = MODULE[cell_type]
    L, r = ops(cell_type, 3, D, 1, half)
    ws = Ws(950, 77) if r.learned else None
    r.fwd(900, D, 901, 902, ws, ST)
    only_call(L, fname, fwant)
    L, r = ops(cell_type, 3, D, 1, half)
    # (the learned cells take no adjoint of rolled-out positions from the module, and have no block partials)
    r.bwd(902, None if r.learned else 903, 904, 905, 906, grads, None if r.learned else 907, ws, 0, ST)
    only_call(L, bname, bwant)


def test_merged_args_are_the_decoder_test_s_rollout_tuple():
    L, r = ops("bouncing_ode_cell", 100, 4, 6, 16.0)
    got = r.merged_args(500, 40, 501, 505)
    assert got == ROLL and [type(a) for a in got] == [type(a) for a in ROLL]
    assert L.calls == []


@pytest.mark.parametrize("cell_type", ["lstm_ode_cell", "interaction_ode_cell"])
def test_a_learned_cell_never_shares_the_decoder_launch(cell_type):
    from paig_reproduction_amd._lib import PaigError
    L, r = ops(cell_type, 100, 4, 6, 16.0)
    with pytest.raises(PaigError):
        r.merged_args(500, 40, 501, 505)
    assert L.calls == []


def test_sizes():
    L, r = ops("spring_ode_cell", 100, 4, 6, 16.0)
    assert (r.workspace_floats(), r.part_doubles()) == (0, 14)
    assert L.calls == [("paig_rollout_bwd_blocks", (100,))]
    L, r = ops("lstm_ode_cell", 100, 4, 6, 16.0)
    assert (r.workspace_floats(), r.part_doubles()) == (1234, 0)
    assert L.calls == [("paig_rollout_lstm_workspace", (100, 4, 100, 6))]
    L, r = ops("interaction_ode_cell", 3, 4, 1, 16.0)
    assert (r.workspace_floats(), r.part_doubles()) == (77, 0)
    assert L.calls == [("paig_rollout_in_workspace", (3, 4, 100, 1))]
    check_signature(*L.calls[0])


def test_engine_workspace_policy():
    """(need_saved, grad_mode) -> whether the engine's forward allocates: the
    LSTM cell whenever a backward may follow, the interaction cell not under
    no_grad, the physics cells never."""
    cases = [(False, False), (False, True), (True, False), (True, True)]
    assert [SPECS["lstm_ode_cell"].saves(*c) for c in cases] == [False, False, True, True]
    assert [SPECS["interaction_ode_cell"].saves(*c) for c in cases] == [False, False, False, True]
    for cell_type in CELL_TYPES[:5]:
        assert not any(SPECS[cell_type].saves(*c) for c in cases)


# ---- the flat buffer's names -----------------------------------------------------------------------------------------
# every name before the cell's: the 32 x 32 and the 36 x 36 frames both take the ShallowUNet
COMMON = [
    "var_net_content.l1.weight", "var_net_content.l1.bias", "var_net_content.l2.weight", "var_net_content.l2.bias",
    "var_net_background.l1.weight", "var_net_background.l1.bias", "var_net_background.l2.weight",
    "var_net_background.l2.bias", "var_net_template.l1.weight", "var_net_template.l1.bias", "var_net_template.l2.weight",
    "var_net_template.l2.bias", "encoder.l1.weight", "encoder.l1.bias", "encoder.l2.weight", "encoder.l2.bias",
    "encoder.shallow_unet.c1.weight", "encoder.shallow_unet.c1.bias", "encoder.shallow_unet.c2.weight",
    "encoder.shallow_unet.c2.bias", "encoder.shallow_unet.c3.weight", "encoder.shallow_unet.c3.bias",
    "encoder.shallow_unet.c4.weight", "encoder.shallow_unet.c4.bias", "encoder.shallow_unet.c5.weight",
    "encoder.shallow_unet.c5.bias", "encoder.shallow_unet.c6.weight", "encoder.shallow_unet.c6.bias",
    "encoder.shallow_unet.c7.weight", "encoder.shallow_unet.c7.bias", "encoder.shallow_unet.c8.weight",
    "encoder.shallow_unet.c8.bias", "encoder.shallow_unet.c9.weight", "encoder.shallow_unet.c9.bias",
    "encoder.shallow_unet.c10.weight", "encoder.shallow_unet.c10.bias", "encoder.shallow_unet.c11.weight",
    "encoder.shallow_unet.c11.bias", "encoder.shallow_unet.c12.weight", "encoder.shallow_unet.c12.bias",
    "encoder.shallow_unet.c13.weight", "encoder.shallow_unet.c13.bias", "encoder.l3.weight", "encoder.l3.bias",
    "velocity_encoder.init_vel_mlp.0.weight", "velocity_encoder.init_vel_mlp.0.bias",
    "velocity_encoder.init_vel_mlp.2.weight", "velocity_encoder.init_vel_mlp.2.bias",
    "velocity_encoder.init_vel_mlp.4.weight", "velocity_encoder.init_vel_mlp.4.bias"]
# cell type -> (task, frame side, the cell's names)
LIVE = {
    "spring_ode_cell": ("spring_color", 32, ["rollout_cell.k", "rollout_cell.equil"]),
    "bouncing_ode_cell": ("bouncing_balls", 32, []),
    "gravity_ode_cell": ("3bp_color", 36, ["rollout_cell.g"]),
    "spring2d_ode_cell": ("spring_color", 32, ["rollout_cell.k", "rollout_cell.equil"]),
    "bouncing2d_ode_cell": ("bouncing_balls", 32, []),
    "lstm_ode_cell": ("spring_color", 32, [
        "rollout_cell.lstm.weight_ih", "rollout_cell.lstm.weight_hh", "rollout_cell.lstm.bias_ih",
        "rollout_cell.lstm.bias_hh", "rollout_cell.proj.weight", "rollout_cell.proj.bias"]),
    "interaction_ode_cell": ("spring_color", 32, [
        "rollout_cell.rel.0.weight", "rollout_cell.rel.0.bias", "rollout_cell.rel.2.weight", "rollout_cell.rel.2.bias",
        "rollout_cell.obj.0.weight", "rollout_cell.obj.0.bias", "rollout_cell.obj.2.weight", "rollout_cell.obj.2.bias"]),
}


def _net(cell_type, **kw):
    task, side, _ = LIVE[cell_type]
    return PhysicsNet(task, 100, 1, cell_type, 12, 4, 6, 3.0, False, True, side * side, "conv_encoder",
                      "conv_st_decoder", **kw)


@pytest.mark.parametrize("cell_type", CELL_TYPES)
def test_live_names(cell_type):
    assert _net(cell_type)._live_names() == COMMON + LIVE[cell_type][2]


def test_live_names_keep_sigma_before_the_cell():
    assert _net("spring_ode_cell", learn_sigma=True)._live_names() == COMMON + ["decoder_sigma_u", "rollout_cell.k",
                                                                               "rollout_cell.equil"]


@pytest.mark.parametrize("cell_type", CELL_TYPES)
def test_spec_agrees_with_its_class(cell_type):
    spec, cls = SPECS[cell_type], getattr(cells, cell_type)
    assert spec.kind == cls.KIND
    cell = cls(4, 4, 100, 16.0) if spec.units_ctor else cls(4, 4)
    params = [cell.get_parameter(n) for n in spec.names]     # every name resolves
    assert all(p.requires_grad for p in params)
    assert {n for n, p in cell.named_parameters() if p.requires_grad} - set(spec.names) <= {
        "weight_ih", "weight_hh", "bias_ih", "bias_hh"}     # (the RNNCell base's unused ones: no gradient, quirk Q8)
    if spec.units_ctor:   # the gradient arguments follow weights()
        assert len(params) == len(cell.weights()) and all(p is w for p, w in zip(params, cell.weights()))
