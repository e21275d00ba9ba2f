"""decoder_ops.DecoderOps on a recording stand-in for the library (no GPU, no
library call): which export every (sigma, targets, operation) the package
uses reaches, and its argument tuple, element by element, against the tuples
the call sites wrote out by hand before DecoderOps existed; each tuple also
against the export's ctypes signature."""
import pytest

from paig_reproduction_amd import _lib
from paig_reproduction_amd.decoder_ops import DecoderOps, Sigma, Targets
from paig_reproduction_amd.engine import LossAdjoints


class RecLib:
    """Records (name, args) of every call; the size queries return SIZES."""
    SIZES = {"paig_decoder_slab_len": 4096, "paig_decoder_bwd_blocks_sigma": 7, "paig_decoder_bwd_scratch_sigma": 11,
             "paig_decoder_bwd_blocks_sigma_dev": 13, "paig_decoder_bwd_scratch_sigma_dev": 17}

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return self.SIZES.get(name, 0)

        return call


class Dev:
    """Stands for a device tensor: only its address is read."""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


K, h, H, FRAME = 2, 16, 32, 3 * 32 * 32
SRC = (101, 102, 103)                      # template, content, background
ST = 9                                     # the stream handle
ROLL_POS = (1000, 28, 4, 6)                # pvs + one step, (R + 1) * 2D, 2D, R
REC_POS = (1000, 0, 4, 0)                  # enc_pos, ungrouped
F32_ROLL = Targets.frames(3000, 50 * FRAME, 6, FRAME)
F32_REC = Targets.frames(3000, 50 * FRAME, 10, FRAME)
U8_ROLL = Targets.dataset_bytes(3300, 3400, 50 * FRAME, 6, FRAME)
ADJ = LossAdjoints(dt=Dev(71), de=None, dr=Dev(73), ae=3, B=100, Te=10, R=6, pred=4)
# engine._rollout_args: (cell, pos0, ld, vel0, dt, p0, p1, pvs, B, D, R); the bouncing cell has no parameters
ROLL = (1, 500, 40, 501, 502, None, None, 505, 100, 4, 6)


def ops(sigma):
    L = RecLib()
    return L, DecoderOps(L, K, h, H, Sigma(sigma), SRC)


def host():
    return ops(0.75)


def device():
    return ops(Dev(777))


def check_signature(name, args):
    """The tuple's length and the Python type of every slot against the
    ctypes table: pointers take int / None, doubles and floats a float, the
    integer kinds an int."""
    argtypes = _lib.SIGNATURES[name][1]
    assert len(args) == len(argtypes), (name, len(args), len(argtypes))
    for i, (a, t) in enumerate(zip(args, argtypes)):
        if t is _lib.P:
            assert a is None or type(a) is int, (name, i, a)
        elif t in (_lib.F64, _lib.F32):
            assert type(a) is float, (name, i, a)
        else:
            assert type(a) is int, (name, i, a)


def only_call(L, name, want):
    assert len(L.calls) == 1, L.calls
    got_name, got = L.calls[0]
    assert got_name == name
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w and type(g) is type(w), (name, i, g, w)
    check_signature(name, got)


# ---- host sigma, fp32 targets (the engine at a fixed log_sig) ---------------
def test_host_f32_forward():
    L, dec = host()
    dec.fwd(ROLL_POS, 2000, FRAME, F32_ROLL, 4000, 600, ST)
    only_call(L, "paig_decoder_fwd_sigma",
              (1000, 28, 4, 6, 101, 102, 103, 2000, 3072, 3000, 153600, 6, 3072, 4000, 600, 2, 16, 32, 0.75, 9))


def test_host_f32_merged_rollout_forward():
    L, dec = host()
    dec.fwd(REC_POS, 2000, FRAME, F32_REC, 4000, 1000, ST, roll=ROLL)
    only_call(L, "paig_decoder_fwd_rollout_sigma",
              (1, 500, 40, 501, 502, None, None, 505, 100, 4, 6,
               1000, 0, 4, 0, 101, 102, 103, 2000, 3072, 3000, 153600, 10, 3072, 4000, 1000, 2, 16, 32, 0.75, 9))


def test_host_f32_backward_inkernel_weights():
    L, dec = host()
    dec.bwd(ROLL_POS, F32_ROLL, None, (2, ADJ), None, FRAME, 5000, 6000, None, 600, 4, ST)
    only_call(L, "paig_decoder_bwd_ex_sigma",
              (1000, 28, 4, 6, 101, 102, 103, 3000, None, None, 153600, 6, 3072, None, 2, 71, None, 73, 3.0, 100, 10, 6, 4,
               None, 3072, 5000, 6000, None, 600, 4, 2, 16, 32, 0.75, 9))


def test_host_f32_backward_weight_array_and_dense_gradient():
    L, dec = host()
    dec.bwd(REC_POS, F32_REC, 7000, None, 8000, FRAME, 5000, 6000, 6500, 1000, 0, ST)
    only_call(L, "paig_decoder_bwd_ex_sigma",
              (1000, 0, 4, 0, 101, 102, 103, 3000, None, None, 153600, 10, 3072, 7000, 0, None, None, None, 0.0, 0, 0, 0,
               0, 8000, 3072, 5000, 6000, 6500, 1000, 0, 2, 16, 32, 0.75, 9))


def test_host_parts():
    L, dec = host()
    dec.parts(1000, 4, 2100, 2200, 50, ST)
    only_call(L, "paig_decoder_parts_sigma", (1000, 4, 101, 102, 103, 2100, 2200, 50, 2, 16, 32, 0.75, 9))


# ---- device sigma, byte targets (the learnable scale over a device-resident dataset) ----
def test_device_bytes_forward():
    L, dec = device()
    dec.fwd(ROLL_POS, 2000, FRAME, U8_ROLL, 4000, 600, ST)
    only_call(L, "paig_decoder_fwd_t8_sigma_dev",
              (1000, 28, 4, 6, 101, 102, 103, 2000, 3072, 3300, 3400, 153600, 6, 3072, 4000, 600, 2, 16, 32, 777, 9))


def test_device_bytes_backward():
    L, dec = device()
    dec.bwd(ROLL_POS, U8_ROLL, 7000, None, None, FRAME, 5000, 6000, 6500, 600, 0, ST, 8800)
    only_call(L, "paig_decoder_bwd_ex_sigma_dev",
              (1000, 28, 4, 6, 101, 102, 103, None, 3300, 3400, 153600, 6, 3072, 7000, 0, None, None, None, 0.0, 0, 0, 0,
               0, None, 3072, 5000, 6000, 6500, 600, 0, 2, 16, 32, 777, 8800, 9))


def test_device_parts():
    L, dec = device()
    dec.parts(1000, 4, 2100, 2200, 50, ST)
    only_call(L, "paig_decoder_parts_sigma_dev", (1000, 4, 101, 102, 103, 2100, 2200, 50, 2, 16, 32, 777, 9))


# ---- device sigma, no targets (the standalone conv_st_decoder) --------------
def test_device_none_forward():
    L, dec = device()
    dec.fwd(REC_POS, 2000, FRAME, Targets.none(), None, 50, ST)
    only_call(L, "paig_decoder_fwd_sigma_dev",
              (1000, 0, 4, 0, 101, 102, 103, 2000, 3072, None, 0, 0, 0, None, 50, 2, 16, 32, 777, 9))


def test_device_none_backward():
    """No targets: the target pointer addresses the dense gradient's frames."""
    L, dec = device()
    dec.bwd(REC_POS, Targets.none(), None, None, 8000, FRAME, 5000, 6000, None, 50, 0, ST, 8800)
    only_call(L, "paig_decoder_bwd_ex_sigma_dev",
              (1000, 0, 4, 0, 101, 102, 103, 8000, None, None, 3072, 0, 0, None, 0, None, None, None, 0.0, 0, 0, 0, 0,
               8000, 3072, 5000, 6000, None, 50, 0, 2, 16, 32, 777, 8800, 9))


def test_host_none_backward_has_no_dsig_slot():
    L, dec = host()
    dec.bwd(REC_POS, Targets.none(), None, None, 8000, FRAME, 5000, 6000, None, 50, 0, ST)
    only_call(L, "paig_decoder_bwd_ex_sigma",
              (1000, 0, 4, 0, 101, 102, 103, 8000, None, None, 3072, 0, 0, None, 0, None, None, None, 0.0, 0, 0, 0, 0,
               8000, 3072, 5000, 6000, None, 50, 0, 2, 16, 32, 0.75, 9))


# ---- sizes ------------------------------------------------------------------
def test_sizes_call_the_query_pair_of_the_sigma_kind():
    L, dec = host()
    assert dec.slab_len == 4096
    assert dec.bwd_sizes(600, 6, 4) == (7, 11)
    assert dec.bwd_sizes(1000) == (7, 11)
    assert L.calls == [("paig_decoder_slab_len", (2, 16, 32)),
                       ("paig_decoder_bwd_blocks_sigma", (600, 6, 4, 2, 16, 32, 0.75)),
                       ("paig_decoder_bwd_scratch_sigma", (600, 2, 16, 32, 0.75)),
                       ("paig_decoder_bwd_blocks_sigma", (1000, 0, 0, 2, 16, 32, 0.75)),
                       ("paig_decoder_bwd_scratch_sigma", (1000, 2, 16, 32, 0.75))]
    L, dec = device()
    assert dec.bwd_sizes(600, 6, 4) == (13, 17)   # every frame walked: no group, no live count
    assert L.calls == [("paig_decoder_bwd_blocks_sigma_dev", (600, 2, 16, 32)),
                       ("paig_decoder_bwd_scratch_sigma_dev", (600, 2, 16, 32))]
    for name, args in L.calls:
        check_signature(name, args)


def test_sigma_kinds():
    s = Sigma(1)   # an integer scale is a host float
    assert (s.on_device, s.suffix, s.has_grad) == (False, "_sigma", False) and type(s.arg) is float and s.arg == 1.0
    t = Dev(777)
    s = Sigma(t)
    assert (s.on_device, s.suffix, s.arg, s.has_grad) == (True, "_sigma_dev", 777, True) and s.value is t


def test_targets_forms():
    assert (F32_ROLL.kind, U8_ROLL.kind, Targets.none().kind) == ("f32", "u8", "none")
    assert (F32_ROLL.value_bytes, U8_ROLL.value_bytes) == (4, 1)
    assert Targets.dataset_bytes(3300, None, FRAME, 0, 0).kind == "u8"   # no row index: sequence q at q * fs
    for bad in (Targets(3000, 3300, None, FRAME, 0, 0), Targets(3000, None, 3400, FRAME, 6, FRAME),
                Targets(None, None, 3400, FRAME, 6, FRAME)):
        with pytest.raises(_lib.PaigError):
            bad.kind


# ---- a Targets of the wrong form raises; it never selects a kernel ----------
@pytest.mark.parametrize("call", [
    lambda dec: dec.fwd(ROLL_POS, 2000, FRAME, U8_ROLL, None, 600, ST),                 # bytes without an SSE output
    lambda dec: dec.fwd(ROLL_POS, 2000, FRAME, Targets.none(), 4000, 600, ST),          # an SSE output without targets
    lambda dec: dec.fwd(REC_POS, 2000, FRAME, U8_ROLL, 4000, 1000, ST, roll=ROLL),      # merged launch: fp32 only
    lambda dec: dec.fwd(REC_POS, 2000, FRAME, Targets.none(), None, 1000, ST, roll=ROLL),
    lambda dec: dec.fwd(ROLL_POS, 2000, FRAME, Targets(3000, 3300, None, FRAME, 0, 0), 4000, 600, ST),
    lambda dec: dec.bwd(ROLL_POS, Targets.none(), None, (2, ADJ), 8000, FRAME, 5000, 6000, None, 600, 0, ST),
    lambda dec: dec.bwd(ROLL_POS, Targets.none(), 7000, None, 8000, FRAME, 5000, 6000, None, 600, 0, ST),
    lambda dec: dec.bwd(ROLL_POS, Targets.none(), None, None, None, FRAME, 5000, 6000, None, 600, 0, ST),
    lambda dec: dec.bwd(ROLL_POS, F32_ROLL, 7000, (2, ADJ), None, FRAME, 5000, 6000, None, 600, 0, ST),
    lambda dec: dec.bwd(ROLL_POS, F32_ROLL, 7000, None, None, FRAME, 5000, 6000, None, 600, 0, ST, 8800),  # host: no dsig
])
def test_wrong_form_raises_without_a_call(call):
    L, dec = host()
    with pytest.raises(_lib.PaigError):
        call(dec)
    assert L.calls == []
