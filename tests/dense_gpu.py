"""Shared plumbing of the direct GPU tests of the dense-tail, velocity-MLP, VFN,
mask-softmax and glue kernels (tests/test_gpu_dense_*.py): guarded NaN-filled
outputs, fp32 device copies at a chosen misalignment, host arrays for the
multi-instance entry points, the 1e-4 normwise comparison with
tests/dense_ref.py, and the expected-error call."""
import ctypes
import math

import pytest
import torch

import dense_ref as R
from helpers import RTOL, rel_err

DEV = torch.device("cuda:0")
HALF = 16.0


def L():
    from paig_reproduction_amd._lib import lib
    return lib()


def st():
    from paig_reproduction_amd._lib import stream_handle
    return stream_handle(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def parr(ts):
    return (ctypes.c_void_p * len(ts))(*[ptr(t) for t in ts])


def iarr(vals):
    return (ctypes.c_int * len(vals))(*vals)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, *shape):
    """fp32 uniform in (-1, 1) on the CPU"""
    return torch.rand(*shape, generator=g) * 2 - 1


def dev(t, off=0):
    """fp32 device copy of a CPU tensor, ``off`` floats into a larger buffer
    (off % 4 != 0: not 16-byte aligned); None stays None."""
    if t is None:
        return None
    t = t.to(torch.float32)
    buf = torch.empty(t.numel() + off, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


class Guard:
    """Output buffers filled with NaN, each followed (and, when offset,
    preceded) by NaN sentinels of at least one row that check() wants intact."""

    def __init__(self):
        self.bufs = []

    def out(self, *shape, off=0):
        n, g = math.prod(shape), max(shape[-1], 4)
        buf = torch.full((off + n + g,), float("nan"), device=DEV)
        self.bufs.append((buf, off, n))
        v = buf[off:off + n].view(*shape)
        assert v.data_ptr() % 16 == (4 * off) % 16
        return v

    def check(self):
        torch.cuda.synchronize()
        for buf, off, n in self.bufs:
            assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all()), \
                "a sentinel beside an output was written"

    def untouched(self):
        """after a refused call: every output still NaN"""
        torch.cuda.synchronize()
        for buf, _, _ in self.bufs:
            assert bool(torch.isnan(buf).all()), "a refused call wrote an output"


def bar(family, key, got, want):
    """got (device fp32) against want (fp64 reference) under the project's
    normwise 1e-4; an unwritten (NaN) element is an infinite error."""
    g = got.detach().double().cpu().reshape(want.shape)
    e = rel_err(g, want)
    print(f"DENSE_ERR {family} {key} {e:.3e}")
    assert e <= RTOL, f"{family} {key}: normwise {e:.3e} > {RTOL:.0e}"
    return e


def same_bits(a, b, what):
    assert a.shape == b.shape and not bool(torch.isnan(a).any()), what
    assert torch.equal(a, b), f"{what}: not bit-identical ({int((a != b).sum())} of {a.numel()} differ)"


def slab_sum(slab, blocks, length):
    """per-block partial rows summed on the host in fp64"""
    assert slab.shape == (blocks, length)
    return slab.double().cpu().sum(0)


def refused(fn, *args):
    """The entry point must refuse these arguments on the host (a non-zero
    status and a message in paig_last_error)."""
    from paig_reproduction_amd._lib import PaigError
    with pytest.raises(PaigError):
        fn(*args)
    assert L().paig_last_error().decode(errors="replace")


# ---------------------------------------------------------------- VFN calls --
VH, VIN = 200, 10


def vfn_inputs(P, seed):
    g = gen(seed)
    return dict(P=P, W1=rnd(g, VH, VIN) * 0.3, b1=rnd(g, VH) * 0.3, W2=rnd(g, P, VH) * 0.1, b2=rnd(g, P), d=rnd(g, P))


def vfn_ref(inst, sig):
    """the float64 forward, the fp32 (h, y) the backward is fed, and its float64 backward"""
    h, y, yp = R.vfn_fwd(*[inst[k].double() for k in ("W1", "b1", "W2", "b2")])
    saved = (h.float(), y.float())
    dW1, db1, dW2, db2, dh = R.vfn_bwd(inst["d"].double(), saved[1].double(), sig, saved[0].double(),
                                       inst["W2"].double())
    return dict(h=h, y=y, ypost=yp, saved=saved, dW1=dW1, db1=db1, dW2=dW2, db2=db2, dh=dh)


def vfn_fwd_args(insts, post, G):
    """(n, W1, b1, W2, b2, hout, y, ypost, P) of paig_vfn_fwd_multi and the
    output views; post[i]: instance i gets a ypost."""
    outs = [dict(h=G.out(VH), y=G.out(i["P"]), ypost=G.out(i["P"]) if p else None) for i, p in zip(insts, post)]
    w = [[dev(i[k]) for i in insts] for k in ("W1", "b1", "W2", "b2")]
    args = (len(insts), *[parr(x) for x in w], parr([o["h"] for o in outs]), parr([o["y"] for o in outs]),
            parr([o["ypost"] for o in outs]), iarr([i["P"] for i in insts]))
    return args, outs, w


def vfn_bwd_args(insts, sig, saved, G):
    """(n, d, y, sig, h, W2, dW1, db1, dW2, db2, part, P) of paig_vfn_bwd*_multi
    and the output views; saved[i] = (h, y) fp32 CPU, made by the reference."""
    Lb = L()
    outs, keep = [], []
    for i in insts:
        P = i["P"]
        nb = Lb.paig_vfn_bwd_blocks(P)
        assert nb == (P + 7) // 8
        outs.append(dict(dW1=G.out(VH, VIN), db1=G.out(VH), dW2=G.out(P, VH), db2=G.out(P), part=G.out(nb, VH)))
    ins = [[dev(i["d"]) for i in insts], [dev(s[1]) for s in saved], [dev(s[0]) for s in saved],
           [dev(i["W2"]) for i in insts]]
    keep.append(ins)
    args = (len(insts), parr(ins[0]), parr(ins[1]), iarr(sig), parr(ins[2]), parr(ins[3]),
            *[parr([o[k] for o in outs]) for k in ("dW1", "db1", "dW2", "db2", "part")], iarr([i["P"] for i in insts]))
    return args, outs, keep
