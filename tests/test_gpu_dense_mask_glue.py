"""The mask softmax (csrc/unet_ops.hip: paig_mask_softmax_fwd / _bwd: the
vector, scalar and pooled kernels, plain and grouped frame views) and the small
glue kernels (paig_pos_head_fwd / _bwd, paig_vel_pack, paig_vel_unpack_add,
paig_colsum) alone, through the C ABI, against the float64 restatements of
tests/dense_ref.py under the project's normwise 1e-4 (helpers.RTOL).  The
backward takes the reference's masks; every output is NaN before the call and
is followed by NaN sentinels that must survive.  The logits hold exact zeros
(a ReLU's output: flag 1 gives an exactly zero gradient there), negative
values and one 90, which overflows fp32 unless the maximum is subtracted."""
import os
import re

import pytest
import torch

import dense_ref as R
from dense_gpu import HALF, Guard, L, bar, dev, gen, ptr, refused, rnd, same_bits, st

pytestmark = pytest.mark.gpu
_id = lambda c: "x".join(map(str, c))   # noqa: E731

#               F  K  C  H  W    vector kernels K = 2, 3 | HW = 15: scalar | K = 1 | K = 7: the local arrays' limit
PLAIN_CASES = [(1, 2, 3, 4, 4), (5, 3, 3, 4, 4), (5, 2, 3, 3, 5), (1, 1, 1, 4, 4), (5, 7, 3, 2, 2)]
POOL_CASES = [(5, 2, 3, 4, 6), (1, 3, 3, 2, 2)]


def _mask_inputs(case, pool=False, grouped=False):
    F, K, C, H, W = case
    g = gen(100 * K + H * W + F)
    lg = rnd(g, F, K, H, W) * 3
    lg[rnd(g, F, K, H, W) > 0.5] = 0.0          # exact zeros (about a quarter), negative values stay
    lg[F - 1, K - 1, H - 1, W - 2] = 90.0
    assert bool((lg == 0).any()) and bool((lg < 0).any())
    d = dict(lg=lg, dobjs=rnd(g, K * F, C, H // 2, W // 2) if pool else rnd(g, K * F, C, H, W))
    if grouped:   # the first Te = 2 frames of each sequence of [B = 2][T = 3][C][H][W]
        assert F == 4
        d["x5"] = rnd(g, 2, 3, C, H, W)
        d["x"] = d["x5"][:, :2].reshape(F, C, H, W)
        d["view"] = (3 * C * H * W, 2, C * H * W)
    else:
        d["x5"] = d["x"] = rnd(g, F, C, H, W)
        d["view"] = (C * H * W, 0, 0)
    return d


def _mask_fwd(case, d, pool=False, off=0):
    """off: logits and masks that many floats into larger buffers"""
    F, K, C, H, W = case
    G = Guard()
    lg, x = dev(d["lg"], off), dev(d["x5"])
    o = dict(masks=G.out(F, K + 1, H, W, off=off), objs=G.out(K * F, C, H, W),
             pobjs=G.out(K * F, C, H // 2, W // 2) if pool else None)
    fs, grp, gs = d["view"]
    L().paig_mask_softmax_fwd(ptr(lg), ptr(x), fs, grp, gs, ptr(o["masks"]), ptr(o["objs"]), ptr(o["pobjs"]), F, K, C,
                              H, W, st())
    G.check()
    return o


def _mask_bwd(case, d, masks, flags, off=0):
    F, K, C, H, W = case
    G = Guard()
    lg, x, m, do = dev(d["lg"], off), dev(d["x5"]), dev(masks, off), dev(d["dobjs"])
    dl = G.out(F, K, H, W)
    fs, grp, gs = d["view"]
    L().paig_mask_softmax_bwd(ptr(lg), ptr(x), fs, grp, gs, ptr(m), ptr(do), ptr(dl), F, K, C, H, W, flags, st())
    G.check()
    return dl


def _check_mask(case, d, pool, off=0):
    ref = R.mask_softmax_fwd(d["lg"].double(), d["x"].double(), pool)
    o = _mask_fwd(case, d, pool, off)
    for k, want in zip(("masks", "objs") + (("pobjs",) if pool else ()), ref):
        bar("mask softmax fwd", k, o[k], want)
    masks32 = ref[0].float()   # the saved masks both sides take
    outs = {}
    for flags in ((2, 3) if pool else (0, 1)):
        want = R.mask_softmax_bwd(d["lg"].double(), d["x"].double(), masks32.double(), d["dobjs"].double(), flags)
        assert float(want.abs().max()) > 0
        dl = _mask_bwd(case, d, masks32, flags, off)
        bar("mask softmax bwd", f"dlogits flags {flags}", dl, want)
        if flags & 1:
            assert bool((dl.cpu()[d["lg"] <= 0] == 0).all()), "flag 1: an exactly zero gradient where the logit is <= 0"
        outs[flags] = dl
    return o, outs


@pytest.mark.parametrize("case", PLAIN_CASES, ids=_id)
def test_mask_softmax(case):
    _check_mask(case, _mask_inputs(case), pool=False)


@pytest.mark.parametrize("case", POOL_CASES, ids=_id)
def test_mask_softmax_pooled(case):
    _check_mask(case, _mask_inputs(case, pool=True), pool=True)


@pytest.mark.parametrize("pool", [False, True])
def test_mask_softmax_grouped_frame_view(pool):
    case = (4, 2, 3, 4, 4)
    _check_mask(case, _mask_inputs(case, pool=pool, grouped=True), pool=pool)


@pytest.mark.parametrize("case", [(1, 2, 3, 4, 4), (5, 3, 3, 4, 4)], ids=_id)
def test_mask_softmax_scalar_kernel_is_bit_identical_to_the_vector_kernel(case):
    """logits and masks one float into larger buffers: not 16-byte aligned, so the scalar kernel runs"""
    d = _mask_inputs(case)
    v, vb = _check_mask(case, d, pool=False)
    s, sb = _check_mask(case, d, pool=False, off=1)
    for k in ("masks", "objs"):
        same_bits(s[k], v[k], k)
    for flags in (0, 1):
        same_bits(sb[flags], vb[flags], f"dlogits flags {flags}")


def test_mask_softmax_eight_objects_are_refused():
    F, K, C, H, W = 1, 8, 3, 2, 2
    g, G = gen(8), Guard()
    lg, x, do = dev(rnd(g, F, K, H, W)), dev(rnd(g, F, C, H, W)), dev(rnd(g, K * F, C, H, W))
    masks, objs, dl = G.out(F, K + 1, H, W), G.out(K * F, C, H, W), G.out(F, K, H, W)
    refused(L().paig_mask_softmax_fwd, ptr(lg), ptr(x), C * H * W, 0, 0, ptr(masks), ptr(objs), None, F, K, C, H, W, st())
    m = dev(rnd(g, F, K + 1, H, W))
    refused(L().paig_mask_softmax_bwd, ptr(lg), ptr(x), C * H * W, 0, 0, ptr(m), ptr(do), ptr(dl), F, K, C, H, W, 0,
            st())
    G.untouched()


# ---------------------------------------------------------------------- glue --
@pytest.mark.parametrize("K", [2, 3])
def test_pos_head(K):
    N = 5
    g, G = gen(K), Guard()
    h3_32, dpos32 = rnd(g, K * N, 2) * 2, rnd(g, N, 2 * K)
    h3, dpos = dev(h3_32), dev(dpos32)
    pos, dh3 = G.out(N, 2 * K), G.out(K * N, 2)
    L().paig_pos_head_fwd(ptr(h3), ptr(pos), N, K, HALF, st())
    L().paig_pos_head_bwd(ptr(h3), ptr(dpos), ptr(dh3), N, K, HALF, st())
    G.check()
    bar("pos head fwd", "pos", pos, R.pos_head_fwd(h3_32.double(), N, K, HALF))
    bar("pos head bwd", "dh3", dh3, R.pos_head_bwd(h3_32.double(), dpos32.double(), N, K, HALF))


@pytest.mark.parametrize("alt", [0, 1])
def test_vel_pack_and_unpack_add(alt):
    B, Te, K, S = 3, 5, 3, 3
    cols = 2 * (S - 1 if alt else S)
    g, G = gen(alt), Guard()
    pos32, dX32, dpos0_32, dpos32 = rnd(g, B, Te, 2 * K), rnd(g, K * B, cols), rnd(g, B, 2 * K), rnd(g, B, Te, 2 * K)
    pos, dX, dpos0 = dev(pos32), dev(dX32), dev(dpos0_32)
    X, dpos = G.out(K * B, cols), G.out(B, Te, 2 * K)
    dpos.copy_(dpos32)
    L().paig_vel_pack(ptr(pos), ptr(X), B, Te, K, S, alt, st())
    L().paig_vel_unpack_add(ptr(dX), ptr(dpos0), ptr(dpos), B, Te, K, S, alt, st())
    G.check()
    bar("vel pack", f"X alt {alt}", X, R.vel_pack(pos32.double(), K, S, alt))
    add = R.vel_unpack(dX32.double(), dpos0_32.double(), B, Te, K, S, alt)
    bar("vel unpack add", f"dpos alt {alt}", dpos, dpos32.double() + add)
    # the matching adjoint: <pack(pos), dX> = <pos, unpack(dX)> on the device's own results
    lhs = float((X.double().cpu() * dX32.double()).sum())
    rhs = float((pos32.double() * R.vel_unpack(dX32.double(), None, B, Te, K, S, alt)).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs), 1.0)
    same_bits(dpos[:, S:].cpu(), dpos32[:, S:], "steps past S untouched")


def _colsum_geometry():
    """the stripe height and the column block of paig_colsum, from its source"""
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "paig_reproduction_amd", "csrc", "unet_ops.hip")).read()
    body = src[src.index("int paig_colsum("):]
    stripe = int(re.search(r"int rows_per = (\d+);", body).group(1))
    block = int(re.search(r"colsum_part_k, dim3\(cdiv\(N, (\d+)\)", body).group(1))
    return stripe, block


@pytest.mark.parametrize("accumulate", [0, 1])
def test_colsum(accumulate):
    stripe, block = _colsum_geometry()
    assert block == 64 and stripe >= 2
    Lb = L()
    for M in (stripe - 1, stripe, stripe + 1):
        for N in (1, 50, block, block + 1):
            g, G = gen(M + N), Guard()
            ld = N + 3
            X32, out0 = rnd(g, M, ld), rnd(g, N)
            X = dev(X32)
            nws = Lb.paig_colsum_workspace(M, N)
            assert nws == -(-M // stripe) * N
            out, ws = G.out(N), G.out(nws)
            if accumulate:   # (else the output stays NaN until the call)
                out.copy_(out0)
            Lb.paig_colsum(ptr(X), M, N, ld, ptr(out), accumulate, ptr(ws), st())
            G.check()
            want = R.colsum(X32[:, :N].double(), out0.double() if accumulate else None)
            bar("colsum", f"M {M} N {N} acc {accumulate}", out, want)
