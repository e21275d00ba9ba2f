"""The grid over which the conv routing queries are characterised
(test_conv_routing.py, test_gpu_conv_refusals.py) and the functions that walk
it.  The recorded answers live in tests/golden/conv_routing.json: plain data,
one entry per point, so that a diff names the point that moved."""
import itertools
import json
import os

CHANNELS = (2, 3, 8, 16, 24, 32, 48, 64, 96, 128)
SIZES = tuple((h, h) for h in (8, 9, 16, 18, 32, 36, 64)) + ((32, 16),)
KS = (1, 3)
ARITH = (0, 128, 256)
FEATURE_BITS = (4, 8, 32, 64, 512)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "conv_routing.json")

UNET_CASES = ((0, 32, 2), (0, 36, 3), (1, 64, 2))   # (net, H, K)
UNET_F = 10
UNET_FLAGS = (1, 1 | 2, 1 | 16, 1 | 32, 1 | 4)


def _subsets(bits):
    return [sum(c) for r in range(len(bits) + 1) for c in itertools.combinations(bits, r)]


def shapes():
    return itertools.product(CHANNELS, CHANNELS, SIZES, KS)


def mfma_accepted(L):
    """[what, Cin, Cout, H, W, ks, flags] of every grid point paig_conv2d_mfma_supported accepts"""
    feats = _subsets(FEATURE_BITS)
    return [[what, ci, co, h, w, ks, a | f]
            for what in (0, 1) for ci, co, (h, w), ks in shapes() for a in ARITH for f in feats
            if L.paig_conv2d_mfma_supported(what, ci, co, h, w, ks, a | f)]


def bwd_accepted(L):
    """[Cin, Cout, H, W, ks, flags] of every grid point paig_conv2d_bwd_supported accepts"""
    feats = _subsets(FEATURE_BITS + (1024,))
    return [[ci, co, h, w, ks, a | f]
            for ci, co, (h, w), ks in shapes() for a in ARITH for f in feats
            if L.paig_conv2d_bwd_supported(ci, co, h, w, ks, a | f)]


def unet_plans(L):
    """{"net H K cm flags": [queries 0..6, workspace bytes, [activation, gradient offset] per buffer]}"""
    out = {}
    for (net, H, K), cm, fl in itertools.product(UNET_CASES, ARITH, UNET_FLAGS):
        q = [int(L.paig_unet_query(net, K, w)) for w in range(7)]
        bufs = [[int(L.paig_unet_buffer(net, UNET_F, H, K, cm, fl, which, b)) for which in (0, 1)]
                for b in range(q[1])]
        out[f"{net} {H} {K} {cm} {fl}"] = [q, int(L.paig_unet_workspace_ex(net, UNET_F, H, K, cm, fl)), bufs]
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
