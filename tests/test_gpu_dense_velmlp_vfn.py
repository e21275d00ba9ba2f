"""The velocity MLP (csrc/velmlp.hip: paig_velmlp_fwd / _bwd / _vfn_fwd) and
VariableFromNetwork (csrc/vfn.h, csrc/misc.hip: paig_vfn_fwd[_multi],
paig_vfn_bwd[_multi], paig_vfn_bwd1_multi) alone, through the C ABI, against
the float64 restatements of tests/dense_ref.py under the project's normwise
1e-4 (helpers.RTOL).  Backwards take the reference's saved activations; every
output is NaN before the call and is followed by NaN sentinels that must
survive; per-block rows are summed on the host in fp64.  The merged launches'
promised bit-identities are checked with torch.equal."""
import pytest
import torch

import dense_ref as R
from dense_gpu import (Guard, L, bar, dev, gen, iarr, parr, ptr, refused, rnd, same_bits, slab_sum, st, vfn_bwd_args,
                       vfn_fwd_args, vfn_inputs, vfn_ref)

pytestmark = pytest.mark.gpu

#             B  Te K  S     2 rows | K = 3, S < Te | IN = 16 = MAXIN | IN = 2
VEL_CASES = [(1, 4, 2, 4), (5, 6, 3, 3), (3, 8, 2, 8), (7, 3, 2, 1)]
HID = R.HID
_id = lambda c: "x".join(map(str, c))   # noqa: E731


def _vel_inputs(case):
    B, Te, K, S = case
    g = gen(100 * B + S)
    W = [rnd(g, HID, 2 * S) / (2 * S) ** 0.5, rnd(g, HID) * 0.1, rnd(g, HID, HID) * 0.15, rnd(g, HID) * 0.1,
         rnd(g, 2, HID) * 0.2, rnd(g, 2) * 0.1]
    return dict(pos=rnd(g, B, Te, 2 * K), W=W, dvel=rnd(g, K * B, 2))


def _vel_ref(case, inp):
    B, Te, K, S = case
    X, h1, h2, vel = R.velmlp_fwd(inp["pos"].double(), K, S, *[w.double() for w in inp["W"]])
    saved = [t.float() for t in (X, h1, h2)]   # what the backward is fed, by kernel and reference alike
    W = inp["W"]
    dX, grads = R.velmlp_bwd(inp["dvel"].double(), *[t.double() for t in saved], W[0].double(), W[2].double(),
                             W[4].double())
    return dict(X=X, h1=h1, h2=h2, vel=vel, saved=saved, dX=dX, grads=grads)


def _vel_fwd(case, inp, w2_off=0, vfn=None):
    """paig_velmlp_fwd, or (vfn = (insts, post)) paig_velmlp_vfn_fwd"""
    B, Te, K, S = case
    rows, G = K * B, Guard()
    W = [dev(w, w2_off if i == 2 else 0) for i, w in enumerate(inp["W"])]
    pos = dev(inp["pos"])
    out = dict(X=G.out(rows, 2 * S), h1=G.out(rows, HID), h2=G.out(rows, HID), vel=G.out(rows, 2))
    a = (ptr(pos), B, Te, K, S, *[ptr(w) for w in W], *[ptr(out[k]) for k in ("X", "h1", "h2", "vel")])
    if vfn is None:
        L().paig_velmlp_fwd(*a, st())
    else:
        va, vo, keep = vfn_fwd_args(*vfn, G)
        L().paig_velmlp_vfn_fwd(*a, *va, st())
        out["vfn"] = vo
    G.check()
    return out


def _vel_bwd(case, inp, saved, w2_off=0):
    B, Te, K, S = case
    rows, G, Lb = K * B, Guard(), L()
    nb, ln = Lb.paig_velmlp_bwd_blocks(rows), Lb.paig_velmlp_slab_len(S)
    assert nb >= 1 and ln == HID * 2 * S + HID + HID * HID + HID + 2 * HID + 2
    W = inp["W"]
    ins = [dev(inp["dvel"])] + [dev(t) for t in saved] + [dev(W[0]), dev(W[2], w2_off), dev(W[4])]
    dX, slab = G.out(rows, 2 * S), G.out(nb, ln)
    Lb.paig_velmlp_bwd(*[ptr(t) for t in ins], ptr(dX), ptr(slab), rows, S, st())
    G.check()
    return dict(dX=dX, slab=slab, nb=nb, ln=ln)


@pytest.mark.parametrize("case", VEL_CASES, ids=_id)
def test_velmlp_forward_and_backward(case):
    inp = _vel_inputs(case)
    ref = _vel_ref(case, inp)
    out = _vel_fwd(case, inp)
    same_bits(out["X"].cpu(), ref["X"].float(), "X is a copy")
    for k in ("X", "h1", "h2", "vel"):
        bar("velmlp fwd", k, out[k], ref[k])
    b = _vel_bwd(case, inp, ref["saved"])
    bar("velmlp bwd", "dX", b["dX"], ref["dX"])
    tot, o = slab_sum(b["slab"], b["nb"], b["ln"]), 0
    for name, want in zip(("W0", "b0", "W2", "b2", "W4", "b4"), ref["grads"]):
        assert float(want.abs().max()) > 0
        bar("velmlp bwd", name, tot[o:o + want.numel()], want)
        o += want.numel()
    assert o == b["ln"]


def test_velmlp_unaligned_w2_is_bit_identical():
    """W2 one float into a larger buffer: the scalar staging path of both kernels"""
    case = (5, 6, 3, 3)
    inp = _vel_inputs(case)
    saved = _vel_ref(case, inp)["saved"]
    a, u = _vel_fwd(case, inp), _vel_fwd(case, inp, w2_off=1)
    for k in ("X", "h1", "h2", "vel"):
        same_bits(u[k], a[k], f"forward {k}")
    ab, ub = _vel_bwd(case, inp, saved), _vel_bwd(case, inp, saved, w2_off=1)
    for k in ("dX", "slab"):
        same_bits(ub[k], ab[k], f"backward {k}")


def test_velmlp_too_many_input_steps_is_refused():
    """S = 9: IN = 18 > MAXIN; a status, a message, nothing written"""
    B, Te, K, S = 2, 9, 2, 9
    g, G, Lb = gen(9), Guard(), L()
    rows = K * B
    W = [dev(w) for w in (rnd(g, HID, 2 * S), rnd(g, HID), rnd(g, HID, HID), rnd(g, HID), rnd(g, 2, HID), rnd(g, 2))]
    pos = dev(rnd(g, B, Te, 2 * K))
    outs = [G.out(rows, 2 * S), G.out(rows, HID), G.out(rows, HID), G.out(rows, 2)]
    refused(Lb.paig_velmlp_fwd, ptr(pos), B, Te, K, S, *[ptr(w) for w in W], *[ptr(o) for o in outs], st())
    ins = [dev(rnd(g, rows, 2)), dev(rnd(g, rows, 2 * S)), dev(rnd(g, rows, HID)), dev(rnd(g, rows, HID))]
    dX, slab = G.out(rows, 2 * S), G.out(Lb.paig_velmlp_bwd_blocks(rows), Lb.paig_velmlp_slab_len(S))
    refused(Lb.paig_velmlp_bwd, *[ptr(t) for t in ins], ptr(W[0]), ptr(W[2]), ptr(W[4]), ptr(dX), ptr(slab), rows, S,
            st())
    G.untouched()


# ----------------------------------------------------------------------- VFN --
def _check_vfn_fwd(out, ref, post):
    for k in ("h", "y") + (("ypost",) if post else ()):
        bar("vfn fwd", k, out[k], ref[k])
    assert post or out["ypost"] is None


def _check_vfn_bwd(out, ref, P):
    for k in ("dW1", "db1", "dW2", "db2"):
        assert float(ref[k].abs().max()) > 0
        bar("vfn bwd", k, out[k], ref[k])
    nb = L().paig_vfn_bwd_blocks(P)
    bar("vfn bwd", "part rows summed", slab_sum(out["part"], nb, R.VH), ref["dh"])


# 4100: past the forward's 1024-block cap (4 rows per block) and 513 > 64 phase-1 partial rows
@pytest.mark.parametrize("P", [1, 3, 8, 9, 288, 4100])
@pytest.mark.parametrize("sig", [0, 1])
def test_vfn_single_instance(P, sig):
    """paig_vfn_fwd / paig_vfn_bwd; the sigmoid instance gets a ypost, the raw one a null ypost"""
    inst = vfn_inputs(P, 7 * P + sig)
    ref = vfn_ref(inst, sig)
    G, Lb = Guard(), L()
    W = [dev(inst[k]) for k in ("W1", "b1", "W2", "b2")]
    out = dict(h=G.out(R.VH), y=G.out(P), ypost=G.out(P) if sig else None)
    Lb.paig_vfn_fwd(*[ptr(w) for w in W], ptr(out["h"]), ptr(out["y"]), ptr(out["ypost"]), P, st())
    G.check()
    _check_vfn_fwd(out, ref, sig)
    (n, d, y, s, h, W2, *o5, Ps), outs, keep = vfn_bwd_args([inst], [sig], [ref["saved"]], G)
    o = outs[0]
    Lb.paig_vfn_bwd(d[0], y[0], sig, h[0], W2[0], *[ptr(o[k]) for k in ("dW1", "db1", "dW2", "db2", "part")], P, st())
    G.check()
    _check_vfn_bwd(o, ref, P)


MULTI_P, MULTI_SIG, MULTI_POST = (9, 4100, 1, 288), (0, 1, 1, 0), (False, True, False, True)


def _multi():
    insts = [vfn_inputs(P, 31 + i) for i, P in enumerate(MULTI_P)]
    return insts, [vfn_ref(i, s) for i, s in zip(insts, MULTI_SIG)]


def test_vfn_four_mixed_instances_in_one_launch():
    insts, refs = _multi()
    G, Lb = Guard(), L()
    fa, fo, keep = vfn_fwd_args(insts, MULTI_POST, G)
    Lb.paig_vfn_fwd_multi(*fa, st())
    G.check()
    for o, r, p in zip(fo, refs, MULTI_POST):
        _check_vfn_fwd(o, r, p)
    ba, bo, keep2 = vfn_bwd_args(insts, MULTI_SIG, [r["saved"] for r in refs], G)
    Lb.paig_vfn_bwd_multi(*ba, st())
    G.check()
    for o, r, P in zip(bo, refs, MULTI_P):
        _check_vfn_bwd(o, r, P)


def test_vfn_five_instances_are_refused():
    insts = [vfn_inputs(3, 50 + i) for i in range(5)]
    refs = [vfn_ref(i, 0) for i in insts]
    G, Lb = Guard(), L()
    fa, _, keep = vfn_fwd_args(insts, [True] * 5, G)
    refused(Lb.paig_vfn_fwd_multi, *fa, st())
    ba, _, keep2 = vfn_bwd_args(insts, [0] * 5, [r["saved"] for r in refs], G)
    refused(Lb.paig_vfn_bwd_multi, *ba, st())
    refused(Lb.paig_vfn_bwd1_multi, *ba, st())
    case = VEL_CASES[0]
    B, Te, K, S = case
    inp = _vel_inputs(case)
    W, pos = [dev(w) for w in inp["W"]], dev(inp["pos"])
    outs = [G.out(K * B, 2 * S), G.out(K * B, HID), G.out(K * B, HID), G.out(K * B, 2)]
    refused(Lb.paig_velmlp_vfn_fwd, ptr(pos), B, Te, K, S, *[ptr(w) for w in W], *[ptr(o) for o in outs], *fa, st())
    G.untouched()


@pytest.mark.parametrize("n", [1, 3])
def test_velmlp_vfn_merged_forward_is_bit_identical(n):
    """paig_velmlp_vfn_fwd against paig_velmlp_fwd followed by paig_vfn_fwd_multi"""
    case = (5, 6, 3, 3)
    inp = _vel_inputs(case)
    insts = [vfn_inputs(P, 60 + i) for i, P in enumerate((9, 4100, 288)[:n])]
    post = (True, False, True)[:n]
    merged = _vel_fwd(case, inp, vfn=(insts, post))
    alone = _vel_fwd(case, inp)
    G = Guard()
    fa, fo, keep = vfn_fwd_args(insts, post, G)
    L().paig_vfn_fwd_multi(*fa, st())
    G.check()
    for k in ("X", "h1", "h2", "vel"):
        same_bits(merged[k], alone[k], k)
    for i, (a, b) in enumerate(zip(merged["vfn"], fo)):
        for k in ("h", "y") + (("ypost",) if post[i] else ()):
            same_bits(a[k], b[k], f"instance {i} {k}")
    ref = _vel_ref(case, inp)
    for k in ("h1", "h2", "vel"):   # the 256-thread blocks of the merged launch, against the reference too
        bar("velmlp fwd", f"merged {k}", merged[k], ref[k])
