"""Refused conv launches: flags 32 (fused upsample input), 64 (fused / folded
max pool) and 512 (transposed-upsample dgrad) exist on the upper kernel tiers
only, and the fused layer backward (paig_conv2d_bwd) has no fallback at all.
For every such point that has no kernel, the public entry point must return
the error code it returned before the kernel routing became one resolver per
family (tests/golden/conv_routing.json, "refusals"), say why
(paig_last_error), report no slab rows, and leave every output -- and the
guards around it -- bit-for-bit untouched.  Nothing is launched on these
calls.  The accepted points are launched and compared with the reference
convolutions by test_gpu_kernels.py, test_gpu_persistent.py,
test_gpu_conv_bwd*.py, test_gpu_conv_fwd_addressing.py and
test_gpu_unet_abi.py."""
import ctypes

import pytest
import torch

import conv_routing_grid as G
from paig_reproduction_amd import _lib

pytestmark = pytest.mark.gpu

CMAX, HMAX, GUARD, NBLK = 128, 64, 256, 4
ACT = CMAX * HMAX * HMAX                  # floats of the largest activation (F = 1)
SLAB = NBLK * (CMAX * CMAX * 9 + CMAX)    # floats of NBLK slab rows of the largest layer
FWD_FEATURES = [f for f in G._subsets((8, 32, 64, 512)) if f & (32 | 64 | 512)] + [4 | 8 | 512]
WG_FEATURES = [f for f in G._subsets((32, 64, 512)) if f]
BWD_FEATURES = G._subsets((32, 64, 1024))


def shapes():
    """(Cin, Cout, H, W, ks) of every shape some query accepts with some flags, in
    both orientations (a dgrad's kernel shape is the layer's transpose), and
    two shapes no list has"""
    g = G.golden()
    s = {tuple(p[1:6]) for p in g["mfma_supported"]} | {tuple(p[0:5]) for p in g["bwd_supported"]}
    s |= {(co, ci, h, w, ks) for ci, co, h, w, ks in s}
    return sorted(s | {(48, 48, 32, 32, 3), (8, 8, 32, 16, 3)})


def candidates(L):
    """(entry, Cin, Cout, H, W, ks, flags) of the points the queries refuse, and
    of the forward points with flags & 512 other than the one form that bit
    has (the split dgrad, no accumulate, upsample or pool): the launch refuses
    those whatever the query says"""
    out = []
    for ci, co, h, w, ks in shapes():
        for a in G.ARITH:
            for f in FWD_FEATURES:
                upt = (f & 512) and not (a == 128 and (f & 8) and not (f & (4 | 32 | 64)))
                if upt or not L.paig_conv2d_mfma_supported(0, ci, co, h, w, ks, a | f):
                    out.append(("fwd", ci, co, h, w, ks, a | f))
            for f in WG_FEATURES:
                if not L.paig_conv2d_mfma_supported(1, ci, co, h, w, ks, a | f):
                    out.append(("wgrad", ci, co, h, w, ks, a | f))
            for f in BWD_FEATURES:
                if not L.paig_conv2d_bwd_supported(ci, co, h, w, ks, a | f):
                    out.append(("bwd", ci, co, h, w, ks, a | f))
    return out


class Arena:
    """Real device operands sized for the largest grid shape at F = 1; the
    outputs (NaN) sit in one buffer between guards, compared whole."""

    def __init__(self):
        dev = torch.device("cuda:0")
        torch.manual_seed(0)
        self.x = torch.rand(ACT, device=dev)
        self.dy = torch.rand(ACT, device=dev)
        self.aux = torch.rand(ACT, device=dev)
        self.w = torch.rand(CMAX * CMAX * 9, device=dev)
        self.bias = torch.rand(CMAX, device=dev)
        names = (("out", ACT), ("slab", SLAB), ("pool", ACT // 4), ("code", ACT // 4))
        total = GUARD + sum(n + GUARD for _, n in names)
        self.outs = torch.empty(total, device=dev)
        self.off, o = {}, GUARD
        for name, n in names:
            self.off[name] = o
            o += n + GUARD
        self.fill()
        self.st = torch.cuda.current_stream().cuda_stream

    def fill(self):
        self.outs.fill_(float("nan"))
        for o in self.off.values():
            self.outs[o - GUARD:o] = 12345.0
        self.outs[-GUARD:] = 12345.0
        self.pristine = self.outs.clone()
        torch.cuda.synchronize()

    def p(self, name):
        return self.outs.data_ptr() + 4 * self.off[name]

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.outs.view(torch.int32), self.pristine.view(torch.int32))

    def call(self, L, entry, ci, co, h, w, ks, flags):
        """-> (return code, *nblk_out or None); the raw C call, F = 1"""
        nb = ctypes.c_int(77)
        x, dy, aux, wt = self.x.data_ptr(), self.dy.data_ptr(), self.aux.data_ptr(), self.w.data_ptr()
        hw = h * w
        if entry == "fwd":
            in_hw = hw // 4 if flags & 32 else hw
            # (the pool operands only with the pool flag: the entry point refuses codes without it)
            pool, code = (self.p("pool"), self.p("code")) if flags & 64 else (None, None)
            rc = L.fns["paig_conv2d_fwd_pwc"](x, ci * in_hw, 0, 0, self.p("out"), co * hw, aux, co * hw, wt,
                                              self.bias.data_ptr(), 1, ci, co, h, w, ks, flags, None, 0,
                                              pool, co * (hw // 4), code, co * (hw // 4), None, self.st)
            return rc, None
        if entry == "wgrad":
            in_hw = hw // 4 if flags & 32 else hw
            rc = L.fns["paig_conv2d_wgrad_ex"](x, ci * in_hw, 0, 0, dy, co * hw, self.p("slab"), NBLK,
                                               ctypes.addressof(nb), 1, ci, co, h, w, ks, flags, None, 0, self.st)
            return rc, nb.value
        in_hw = hw // 4 if flags & 32 else hw
        rc = L.fns["paig_conv2d_bwd"](x, ci * in_hw, 0, 0, dy, co * hw, self.p("out"), ci * in_hw, aux, ci * in_hw,
                                      wt, self.p("slab"), NBLK, ctypes.addressof(nb), 1, ci, co, h, w, ks, flags,
                                      None, 0, self.p("pool"), co * (hw // 4), self.p("code"), co * (hw // 4) // 8 * 8,
                                      None, self.st)
        return rc, nb.value


def test_refused_points_keep_their_code_and_touch_nothing():
    L = _lib.lib()
    want = {tuple(p[:-1]): p[-1] for p in G.golden()["refusals"]}
    # the recorded table is this grid's refusals, nothing else
    assert set(want) <= set(candidates(L)), sorted(set(want) - set(candidates(L)))[:20]
    assert {c for c in want.values()} <= {1001, 1002}
    arena = Arena()
    bad = []
    for point, code in want.items():
        rc, nb = arena.call(L, *point)
        msg = L.fns["paig_last_error"]()
        ok = rc == code and bool(msg) and nb in (None, 0) and arena.untouched()
        if not ok:
            bad.append((point, code, rc, nb, msg))
            print("point", point, "recorded", code, "returned", rc, "nblk_out", nb, "error", msg)
            arena.fill()
    assert not bad, f"{len(bad)} of {len(want)} refused points moved"
