"""The localiser's dense tail and position head (csrc/velmlp.hip:
paig_dense_tail_fwd, paig_head_fwd, paig_head_bwd, paig_head_bwd_vel,
paig_head_bwd_vel_vfn2, paig_head_l2_bwd) and the split-K slabs that feed the
tail (csrc/gemm.hip: paig_gemm_parts, paig_gemm_parts_size) alone, through the
C ABI, against the float64 restatements of tests/dense_ref.py under the
project's normwise 1e-4 (helpers.RTOL).  Backwards take saved activations made
by the reference (exact zeros in about half of h1 / h2, where the gradients
must be exactly 0.0); every output is NaN before the call and is followed by
NaN sentinels that must survive; slab rows are summed on the host in fp64.
The header's bit-identity promises are checked with torch.equal."""
import types

import pytest
import torch

import dense_ref as R
from dense_gpu import (HALF, Guard, L, bar, dev, gen, iarr, parr, ptr, refused, rnd, same_bits, slab_sum, st,
                       vfn_bwd_args, vfn_inputs, vfn_ref)

pytestmark = pytest.mark.gpu
_id = lambda c: "x".join(map(str, c))   # noqa: E731


def _relu_act(g, *shape):
    """a ReLU's output: exact zeros in about half the entries"""
    t = torch.relu(rnd(g, *shape))
    assert 0.3 < float((t == 0).float().mean()) < 0.7 or t.numel() < 16
    return t


# ---------------------------------------------------------------- dense tail --
#              K  F  IN   S     rows 2 | 15 = 8 + 7, K = 3 | 16;  S around the 8-slab loop;  IN masks
TAIL_CASES = [(2, 1, 4, 1), (3, 5, 20, 7), (2, 8, 24, 8), (3, 5, 196, 9), (2, 8, 200, 17), (3, 5, 200, 8),
              (2, 1, 200, 9), (2, 8, 4, 17), (3, 5, 24, 1)]


def _tail_inputs(case):
    K, F, IN, S = case
    g = gen(1000 * IN + 10 * S + F)
    return dict(part=rnd(g, S, K * F, IN), b1=rnd(g, IN) * 0.2, W2=rnd(g, IN, IN) / IN ** 0.5, b2=rnd(g, IN) * 0.2,
                W3=rnd(g, 2, IN) / IN ** 0.5, b3=rnd(g, 2) * 0.2)


def _tail_fwd(case, inp, part=None, w2t=None):
    """paig_dense_tail_fwd with W2 (transposed by the call) or, w2t given, with W2 = NULL"""
    K, F, IN, S = case
    G = Guard()
    o = dict(h1=G.out(K * F, IN), h2=G.out(K * F, IN), h3=G.out(K * F, 2), pos=G.out(F, 2 * K))
    w = {k: dev(inp[k]) for k in ("b1", "W2", "b2", "W3", "b3")}
    part = dev(inp["part"]) if part is None else part
    scratch = G.out(IN, IN) if w2t is None else w2t
    L().paig_dense_tail_fwd(ptr(part), S, ptr(w["b1"]), ptr(o["h1"]), ptr(w["W2"]) if w2t is None else None,
                            ptr(scratch), ptr(w["b2"]), ptr(o["h2"]), ptr(w["W3"]), ptr(w["b3"]), ptr(o["h3"]),
                            ptr(o["pos"]), F, K, IN, HALF, st())
    G.check()
    o["W2t"] = scratch
    return o


@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_dense_tail_forward(case):
    K, F, IN, S = case
    inp = _tail_inputs(case)
    ref = R.dense_tail_fwd(*[inp[k].double() for k in ("part", "b1", "W2", "b2", "W3", "b3")], F, K, HALF)
    out = _tail_fwd(case, inp)
    for k, want in zip(("h1", "h2", "h3", "pos"), ref):
        bar("dense tail fwd", k, out[k], want)
    same_bits(out["W2t"].cpu(), inp["W2"].T.contiguous(), "W2t = W2^T")
    # the header's order: the slabs added in slab order, then b1, then the ReLU (fp32, reproducible on the CPU)
    acc = inp["part"][0].clone()
    for s in range(1, S):
        acc = acc + inp["part"][s]
    same_bits(out["h1"].cpu(), torch.relu(acc + inp["b1"]), "h1 in slab order")
    assert K * F < 8 or 0.2 < float((ref[0] == 0).double().mean()) < 0.8   # the ReLU decides something


@pytest.mark.parametrize("case", [(3, 5, 24, 9), (2, 8, 200, 7)], ids=_id)
def test_dense_tail_prepared_w2t_is_bit_identical(case):
    """W2 = NULL with the W2^T image of paig_conv_wprep's dg = 2 job"""
    K, F, IN, S = case
    inp = _tail_inputs(case)
    a = _tail_fwd(case, inp)
    G = Guard()
    W2, w2t = dev(inp["W2"]), G.out(IN, IN)
    L().paig_conv_wprep(1, parr([W2]), iarr([IN]), iarr([IN]), iarr([1]), iarr([2]), parr([w2t]), st())
    G.check()
    same_bits(w2t, a["W2t"], "the prepared W2^T")
    b = _tail_fwd(case, inp, w2t=w2t)
    for k in ("h1", "h2", "h3", "pos"):
        same_bits(b[k], a[k], k)


@pytest.mark.parametrize("IN,off", [(6, 0), (204, 0), (8, 1)])
def test_dense_tail_unsupported_arguments_are_refused(IN, off):
    """IN no multiple of 4, IN > 200, a W2t that is not 16-byte aligned"""
    K, F, S = 2, 3, 2
    g, G = gen(3), Guard()
    o = [G.out(K * F, IN), G.out(K * F, IN), G.out(K * F, 2), G.out(F, 2 * K)]
    w2t = G.out(IN, IN, off=off)
    part, b1, W2, b2, W3, b3 = (dev(rnd(g, *s)) for s in ((S, K * F, IN), (IN,), (IN, IN), (IN,), (2, IN), (2,)))
    refused(L().paig_dense_tail_fwd, ptr(part), S, ptr(b1), ptr(o[0]), ptr(W2), ptr(w2t), ptr(b2), ptr(o[1]), ptr(W3),
            ptr(b3), ptr(o[2]), ptr(o[3]), F, K, IN, HALF, st())
    G.untouched()


# ---------------------------------------------------------------- gemm parts --
def _engine_math():
    """the two arithmetic modes the engine passes for the forward l1 GEMM"""
    from paig_reproduction_amd.engine import Engine
    out = []
    for m in ("split", "fp32"):
        eng = types.SimpleNamespace(model=types.SimpleNamespace(conv_math=m), GEMM_MATH=Engine.GEMM_MATH)
        out.append(Engine.gemm_math(eng, Engine.FWD))
    assert len(set(out)) == 2
    return out


def _parts(M, N, Kd, A, B, math, floats, G):
    """paig_gemm_parts into a NaN buffer of ``floats`` -> (S, buffer)"""
    buf = G.out(floats)
    S = L().paig_gemm_parts(0, 1, M, N, Kd, ptr(A), Kd, ptr(B), Kd, ptr(buf), floats, math, st())
    G.check()
    return S, buf


@pytest.mark.parametrize("shape", [(74, 200, 3072), (16, 200, 64)], ids=_id)
@pytest.mark.parametrize("mode", [0, 1])
def test_gemm_parts(shape, mode):
    M, N, Kd = shape
    math = _engine_math()[mode]
    g, G, Lb = gen(M + mode), Guard(), L()
    A32, B32 = rnd(g, M, Kd), rnd(g, N, Kd) / Kd ** 0.5
    A, B = dev(A32), dev(B32)
    want = A32.double() @ B32.double().T
    need = Lb.paig_gemm_parts_size(M, N, Kd, math)
    assert need >= M * N and need % (M * N) == 0
    S, buf = _parts(M, N, Kd, A, B, math, need, G)
    assert 1 <= S <= need // (M * N), f"S = {S} (status {-S if S < 0 else 0}: {Lb.paig_last_error()})"
    slabs = buf[:S * M * N].view(S, M, N)
    bar("gemm parts", f"math {math} sum of {S} slabs", slabs.double().sum(0), want)
    assert bool(torch.isnan(buf[S * M * N:]).all())
    # fewer floats than the plan's split, at least one slab: S = 1, the same product
    S1, buf1 = _parts(M, N, Kd, A, B, math, M * N + (1 if need > M * N else 0), G)
    assert S1 == 1
    bar("gemm parts", f"math {math} one slab", buf1[:M * N], want)
    # less than one slab: a negative status, nothing written
    G2 = Guard()
    small = G2.out(M * N)
    rc = Lb.paig_gemm_parts(0, 1, M, N, Kd, ptr(A), Kd, ptr(B), Kd, ptr(small), M * N - 1, math, st())
    assert rc < 0 and Lb.paig_last_error()
    G2.untouched()


def test_gemm_parts_slabs_into_dense_tail():
    """the real l1 slabs (74 rows x 3072 inputs) through the tail, end to end"""
    K, F, IN, n1 = 2, 37, 200, 3072
    math = _engine_math()[0]
    g, G, Lb = gen(74), Guard(), L()
    x, W1 = torch.relu(rnd(g, K * F, n1)), rnd(g, IN, n1) / n1 ** 0.5 * 3
    need = Lb.paig_gemm_parts_size(K * F, IN, n1, math)
    S, buf = _parts(K * F, IN, n1, dev(x), dev(W1), math, need, G)
    assert S >= 1
    inp = _tail_inputs((K, F, IN, 1))
    out = _tail_fwd((K, F, IN, S), inp, part=buf)
    part = (x.double() @ W1.double().T)[None]
    ref = R.dense_tail_fwd(part, *[inp[k].double() for k in ("b1", "W2", "b2", "W3", "b3")], F, K, HALF)
    for k, want in zip(("h1", "h2", "h3", "pos"), ref):
        bar("gemm parts -> dense tail", k, out[k], want)


# ---------------------------------------------------------------------- head --
#              K  F   IN     rows 2, 15, 16, 17, 33 (16 per backward block); IN 260 > the 256-thread block
HEAD_CASES = [(2, 1, 4), (3, 5, 200), (2, 8, 260), (1, 17, 200), (3, 11, 260), (3, 11, 4), (1, 17, 4), (2, 1, 260)]


def _head_inputs(K, F, IN, seed=0):
    g = gen(100 * IN + F + seed)
    d = dict(h2=_relu_act(g, K * F, IN), W3=rnd(g, 2, IN) / IN ** 0.5 * 2, b3=rnd(g, 2) * 0.2, dpos=rnd(g, F, 2 * K),
             h1=_relu_act(g, K * F, IN), W2=rnd(g, IN, IN) / IN ** 0.5)
    h3, _ = R.head_fwd(d["h2"].double(), d["W3"].double(), d["b3"].double(), F, K, HALF)
    d["h3"] = h3.float()   # the saved activation both sides take
    return d


def _head_ref(d, K, F, vel=None):
    v = None if vel is None else tuple(None if t is None else t.double() for t in vel[:2]) + tuple(vel[2:])
    dh2, dW3, db3 = R.head_bwd(d["h2"].double(), d["h3"].double(), d["dpos"].double(), d["W3"].double(), F, K, HALF, v)
    return dict(dh2=dh2, slab=torch.cat([dW3.reshape(-1), db3]), dh1=R.l2_bwd(dh2, d["W2"].double(), d["h1"].double()))


def _head_bwd(d, K, F, IN, entry="plain", vel=None, vfn=None, dpos=None, w2_off=0, G=None):
    """entry: plain (paig_head_bwd), vel (paig_head_bwd_vel), vfn2
    (paig_head_bwd_vel_vfn2), l2 (paig_head_l2_bwd).  vel = (dX, dpos0, B, Te,
    S, alt) CPU tensors or None; vfn: paig_vfn_bwd*_multi's argument tuple."""
    Lb, G = L(), G or Guard()
    l2 = entry == "l2"
    nb = (Lb.paig_head_l2_bwd_blocks if l2 else Lb.paig_head_bwd_blocks)(K * F)
    assert nb == -(-K * F // (8 if l2 else 16))
    ins = [dev(d["h2"]), dev(d["h3"]), dev(d["dpos"]) if dpos is None else dpos, dev(d["W3"])]
    o = dict(dh2=G.out(K * F, IN), slab=G.out(nb, 2 * IN + 2), nb=nb)
    a = (*[ptr(t) for t in ins], ptr(o["dh2"]), ptr(o["slab"]), F, K, IN, HALF)
    keep = [dev(vel[0]), dev(vel[1])] if vel else [None, None]
    va = (ptr(keep[0]), ptr(keep[1]), *vel[2:]) if vel else (None, None, 0, 0, 0, 0)
    if entry == "plain":
        Lb.paig_head_bwd(*a, st())
    elif entry == "vel":
        Lb.paig_head_bwd_vel(*a, *va, st())
    elif entry == "vfn2":
        Lb.paig_head_bwd_vel_vfn2(*a, *va, *vfn, st())
    else:
        o["dh1"] = G.out(K * F, IN)
        W2, h1 = dev(d["W2"], w2_off), dev(d["h1"])
        Lb.paig_head_l2_bwd(*a, *va, ptr(W2), ptr(h1), ptr(o["dh1"]), *(vfn if vfn else (0,) + (None,) * 11), st())
    G.check()
    return o


def _check_head(o, ref, d, IN, family, l2=False):
    bar(family, "dh2", o["dh2"], ref["dh2"])
    assert bool((o["dh2"].cpu()[d["h2"] == 0] == 0).all()), "dh2 must be exactly 0.0 where h2 is"
    bar(family, "[W3|b3]", slab_sum(o["slab"], o["nb"], 2 * IN + 2), ref["slab"])
    if l2:
        bar(family, "dh1", o["dh1"], ref["dh1"])
        assert bool((o["dh1"].cpu()[d["h1"] == 0] == 0).all()), "dh1 must be exactly 0.0 where h1 is"


@pytest.mark.parametrize("case", HEAD_CASES, ids=_id)
def test_head_forward_and_backward(case):
    K, F, IN = case
    d = _head_inputs(K, F, IN)
    G = Guard()
    h3, pos = G.out(K * F, 2), G.out(F, 2 * K)
    ins = [dev(d[k]) for k in ("h2", "W3", "b3")]
    L().paig_head_fwd(*[ptr(t) for t in ins], ptr(h3), ptr(pos), F, K, IN, HALF, st())
    G.check()
    rh3, rpos = R.head_fwd(d["h2"].double(), d["W3"].double(), d["b3"].double(), F, K, HALF)
    bar("head fwd", "h3", h3, rh3)
    bar("head fwd", "pos", pos, rpos)
    _check_head(_head_bwd(d, K, F, IN), _head_ref(d, K, F), d, IN, "head bwd")


def _vel_term(K, B, Te, S, alt, which, seed=0):
    g = gen(17 * K + 3 * alt + which + seed)
    cols = 2 * (S - 1 if alt else S)
    return (rnd(g, K * B, cols) if which & 1 else None, rnd(g, B, 2 * K) if which & 2 else None, B, Te, S, alt)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("alt", [0, 1])
@pytest.mark.parametrize("which", [1, 2, 3], ids=["dX", "dpos0", "both"])
def test_head_backward_with_velocity_term(K, alt, which):
    """paig_head_bwd_vel against the reference, and bit for bit against
    paig_vel_unpack_add into a copy of dpos followed by paig_head_bwd"""
    B, Te, S, IN = 3, 5, 3, 200
    F = B * Te
    d = _head_inputs(K, F, IN, seed=alt)
    vel = _vel_term(K, B, Te, S, alt, which)
    o = _head_bwd(d, K, F, IN, "vel", vel)
    _check_head(o, _head_ref(d, K, F, vel), d, IN, "head bwd vel")
    plain = _head_ref(d, K, F)
    assert float((plain["dh2"] - _head_ref(d, K, F, vel)["dh2"]).abs().max()) > 1e-3   # the term matters
    G = Guard()
    dpos = G.out(F, 2 * K)
    dpos.copy_(d["dpos"])
    dX, dpos0 = dev(vel[0]), dev(vel[1])
    L().paig_vel_unpack_add(ptr(dX), ptr(dpos0), ptr(dpos), B, Te, K, S, alt, st())
    two = _head_bwd(d, K, F, IN, "plain", dpos=dpos, G=G)
    same_bits(o["dh2"], two["dh2"], "dh2")
    same_bits(o["slab"], two["slab"], "slab")


#            K  F  B  Te S  IN    rows 2, 15, 16 (8 per block)
L2_CASES = [(2, 1, 1, 1, 1, 4), (3, 5, 1, 5, 3, 24), (2, 8, 2, 4, 3, 200), (3, 5, 1, 5, 3, 200), (2, 8, 2, 4, 3, 4),
            (2, 1, 1, 1, 1, 24)]


def _vfn_pair(G):
    """two VFN instances after their phase 1 alone, and after the whole backward"""
    insts, sig = [vfn_inputs(P, 90 + P) for P in (4100, 9)], [1, 0]
    saved = [vfn_ref(i, s)["saved"] for i, s in zip(insts, sig)]
    whole_a, whole_o, k1 = vfn_bwd_args(insts, sig, saved, G)
    L().paig_vfn_bwd_multi(*whole_a, st())
    ph1_a, ph1_o, k2 = vfn_bwd_args(insts, sig, saved, G)
    L().paig_vfn_bwd1_multi(*ph1_a, st())
    torch.cuda.synchronize()   # phase 1 alone leaves the first layer's gradients to phase 2
    assert all(bool(torch.isnan(o[k]).all()) for o in ph1_o for k in ("dW1", "db1"))
    return ph1_a, ph1_o, whole_o, (k1, k2)


def _same_vfn(ph1_o, whole_o):
    for i, (a, b) in enumerate(zip(ph1_o, whole_o)):
        for k in ("dW1", "db1", "dW2", "db2", "part"):
            same_bits(a[k], b[k], f"VFN instance {i} {k}")


@pytest.mark.parametrize("case", L2_CASES, ids=_id)
@pytest.mark.parametrize("with_vel", [0, 1])
def test_head_l2_backward(case, with_vel):
    """n = 0 on the cases without the velocity term, n = 2 (the VFN backward's
    phase 2 in the same launch) on those with it"""
    K, F, B, Te, S, IN = case
    d = _head_inputs(K, F, IN, seed=with_vel)
    vel = _vel_term(K, B, Te, S, 0, 3, seed=F) if with_vel else None
    G = Guard()
    vfn = _vfn_pair(G) if with_vel else None
    o = _head_bwd(d, K, F, IN, "l2", vel, vfn=vfn[0] if vfn else None, G=G)
    _check_head(o, _head_ref(d, K, F, vel), d, IN, "head l2 bwd", l2=True)
    if vfn:
        _same_vfn(vfn[1], vfn[2])
    ref_entry = _head_bwd(d, K, F, IN, "vel", vel) if with_vel else _head_bwd(d, K, F, IN, "plain")
    same_bits(o["dh2"], ref_entry["dh2"], "dh2 against paig_head_bwd_vel's")


def test_head_vfn2_phase2_is_bit_identical():
    """paig_vfn_bwd1_multi then the phase-2 blocks of paig_head_bwd_vel_vfn2:
    the same bits as paig_vfn_bwd_multi, and the head part as paig_head_bwd_vel"""
    K, B, Te, S, IN = 3, 3, 5, 3, 200
    F = B * Te
    d, vel = _head_inputs(K, F, IN), _vel_term(K, B, Te, S, 1, 3)
    G = Guard()
    ph1_a, ph1_o, whole_o, keep = _vfn_pair(G)
    o = _head_bwd(d, K, F, IN, "vfn2", vel, vfn=ph1_a, G=G)
    _same_vfn(ph1_o, whole_o)
    _check_head(o, _head_ref(d, K, F, vel), d, IN, "head bwd vel vfn2")
    alone = _head_bwd(d, K, F, IN, "vel", vel)
    same_bits(o["dh2"], alone["dh2"], "dh2")
    same_bits(o["slab"], alone["slab"], "slab")


def test_head_l2_unaligned_w2_is_refused():
    K, F, IN = 2, 3, 8
    d = _head_inputs(K, F, IN)
    from paig_reproduction_amd._lib import PaigError
    G = Guard()
    with pytest.raises(PaigError):
        _head_bwd(d, K, F, IN, "l2", w2_off=1, G=G)
    assert L().paig_last_error()
    G.untouched()
