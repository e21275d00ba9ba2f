"""dL/dsigma of the generic decoder backward with sigma in device memory
(paig_decoder_bwd_ex_sigma_dev), and the two small kernels around it
(paig_sigma_from_u, paig_sigma_grad), directly through the C ABI.

The reference cannot produce dL/dsigma (its sigma is a Python float), so the
yardstick is float64 autograd through tests/sigma_grad_ref.py, with one sigma
per frame so that one backward yields every dsig_f.

Bar (the project's envelope rule, tests/envelope.py): the kernel's error
against float64 <= max(ENVELOPE_K x the error of the fp32 autograd run of the
same helper against float64, ENVELOPE_FLOOR), errors relative to max_f
|dsig_f|; for every dsig_f and for their sum.  Non-vacuity is asserted on the
float64 reference before the kernel is looked at: |sum_f dsig_f| >= 0.05 sum_f
|dsig_f| and max_f |dsig_f| > 0; the positions' seed is the first for which
that holds and no sampling coordinate lies within 1e-3 px of an integer (the
bilinear derivative jumps there, as in test_gpu_sigma_decoder.py).

Also: with dsig given, dpos and the slab rows are bit-identical to the launch
without it, and (sigma = 0.6) to paig_decoder_bwd_ex_sigma, which takes the same
generic kernel below sigma = 1; dead frames (NaN targets) get dsig exactly
0.0; two launches give the same bits.  Measured: DESIGN.md section 4b, "Learnable decoder window scale".
"""
import functools
import types

import numpy as np
import pytest
import torch

from envelope import ENVELOPE_FLOOR, ENVELOPE_K
import sigma_grad_ref as SG
import sigma_ref as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CU_SHAPES = [(2, 32), (3, 36), (2, 64)]        # byte targets / in-kernel weights: these only (dec_bwd's rule)
SHAPES = CU_SHAPES + [(2, 16)]
SIGMAS = [0.6, 1.0, 1.7]
NAN = float("nan")


def L():
    from paig_reproduction_amd._lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def p_(t):
    return None if t is None else t.data_ptr()


def _cfg(K, H):
    return types.SimpleNamespace(n_objs=K, tmpl=H // 2, size=H)


def _sources(K, H, seed):
    g = torch.Generator().manual_seed(seed)
    h = H // 2
    return (torch.randn(K, 1, h, h, generator=g) * 2.0, torch.randn(K, 3, h, h, generator=g),
            torch.sigmoid(torch.randn(1, 3, H, H, generator=g)))


def _u8_targets(n, H, seed):
    u8 = torch.randint(0, 256, (n, 3, H, H), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return u8, u8.float() / 255.0


def _autograd(K, H, sigma, src, pos, tgt, w, dout, dtype):
    """Every frame's dL/dsigma_f of L = sum_f w_f ||out_f - tgt_f||^2 + <dout,
    out> by autograd in ``dtype`` (sigma itself a float64 leaf, one per frame)."""
    tmpl, cont, bg = (t.to(dtype) for t in src)
    sg = torch.full((pos.shape[0],), float(sigma), dtype=torch.float64, requires_grad=True)
    joint = torch.cat([tmpl.repeat(1, 3, 1, 1) + 5, torch.sigmoid(cont)], 1)
    out = SG.st_decoder_sigma(_cfg(K, H), joint, bg, pos.to(dtype), sg)
    loss = 0.0
    if w is not None:
        loss = loss + (w.to(dtype).view(-1, 1, 1, 1) * (out - tgt.to(dtype)) ** 2).sum()
    if dout is not None:
        loss = loss + (out * dout.to(dtype)).sum()
    loss.backward()
    return sg.grad.detach().numpy().copy()


@functools.lru_cache(maxsize=None)
def _case(K, H, sigma, n, kind, grouped):
    """(positions, targets u8 / fp32, weights, dense dout, float64 reference,
    fp32 reference) of one case, from the first seed whose float64 reference is
    tie-free and non-vacuous.  Frame 0's objects sit near the centre; the others
    are spread over (-0.25 H, 1.25 H): partly and wholly outside the frame."""
    src = _sources(K, H, 10 * K + H)
    u8, tgt = _u8_targets(n, H, 99)
    B, R, live = 3, 4, 2
    if kind == "dense":
        w, dout = None, torch.randn(n, 3, H, H, generator=torch.Generator().manual_seed(4))
    else:
        dout = None
        if kind == "lw":      # the in-kernel weights' values (test_gpu_sigma_decoder.py's adjoints)
            w = torch.full((n,), 0.37 / n) if not grouped else torch.full((B, R), 0.83 / (B * live))
        else:
            w = torch.rand(n if not grouped else (B, R), generator=torch.Generator().manual_seed(7)) + 0.1
        if grouped:
            w = w.view(B, R).clone()
            w[:, live:] = 0.0
            w = w.reshape(-1)
    for seed in range(1, 400):
        g = torch.Generator().manual_seed(seed)
        pos = (torch.rand(n, 2 * K, generator=g) * 1.5 - 0.25) * H
        pos[0] = H / 2 + (torch.rand(2 * K, generator=g) - 0.5) * 3.0
        c = SR.sample_coords(K, H, pos, SR.sigma_of(sigma))
        if (c - torch.round(c)).abs().min().item() <= 1e-3:
            continue
        r64 = _autograd(K, H, sigma, src, pos, tgt, w, dout, torch.float64)
        if np.abs(r64).max() > 0 and abs(r64.sum()) >= 0.05 * np.abs(r64).sum():
            r32 = _autograd(K, H, sigma, src, pos, tgt, w, dout, torch.float32)
            return src, pos, u8, tgt, w, dout, r64, r32
    raise AssertionError("no seed with a tie-free, non-vacuous reference")


def _launch(K, H, src, pv, tv, F_, live=0, tgt=None, tgt8=None, w=None, lw=None, dout=None, sigma_dev=None,
            host_sigma=None, want_dsig=True):
    """paig_decoder_bwd_ex_sigma_dev (or, host_sigma, paig_decoder_bwd_ex_sigma):
    (dpos, slab rows, dsig or None), NaN-prefilled."""
    h = H // 2
    lib = L()
    td, cd, bd = (s.to(DEV).contiguous() for s in src)
    slab_len = int(lib.paig_decoder_slab_len(K, h, H))
    if host_sigma is None:
        nb, scr_n = lib.paig_decoder_bwd_blocks_sigma_dev(F_, K, h, H), lib.paig_decoder_bwd_scratch_sigma_dev(F_, K, h, H)
    else:
        nb = lib.paig_decoder_bwd_blocks_sigma(F_, pv[3], live, K, h, H, host_sigma)
        scr_n = lib.paig_decoder_bwd_scratch_sigma(F_, K, h, H, host_sigma)
    assert nb == max((F_ + 1) // 2, 1)
    slab = torch.full((nb * slab_len,), NAN, device=DEV)
    scratch = torch.empty(scr_n, device=DEV) if scr_n else None
    dpos = torch.full((F_, 2 * K), NAN, device=DEV)
    dsig = torch.full((F_,), NAN, device=DEV, dtype=torch.float64) if (want_dsig and host_sigma is None) else None
    wd = w.to(DEV) if w is not None else None
    dd = dout.to(DEV).contiguous() if dout is not None else None
    keep = []
    if lw is not None:
        mode, adj, lB, lTe, lR, lpred = lw
        ad = torch.tensor([adj], device=DEV)
        keep.append(ad)
        lwa = (mode, p_(ad) if mode == 2 else None, None, p_(ad) if mode == 1 else None, 0.0, lB, lTe, lR, lpred)
    else:
        lwa = (0, None, None, None, 0.0, 0, 0, 0, 0)
    args = (*pv, p_(td), p_(cd), p_(bd), tgt, tgt8, None, *tv, p_(wd), *lwa, p_(dd), 3 * H * H, p_(dpos), p_(slab),
            p_(scratch), F_, live, K, h, H)
    if host_sigma is None:
        lib.paig_decoder_bwd_ex_sigma_dev(*args, p_(sigma_dev), p_(dsig), st())
    else:
        lib.paig_decoder_bwd_ex_sigma(*args, host_sigma, st())
    torch.cuda.synchronize()
    return dpos.cpu(), slab.cpu(), None if dsig is None else dsig.cpu().numpy()


def _judge(got, r64, r32, what):
    scale = np.abs(r64).max()
    rows = {"per-frame": (np.abs(got - r64).max() / scale, np.abs(r32 - r64).max() / scale),
            "sum": (abs(got.sum() - r64.sum()) / scale, abs(r32.sum() - r64.sum()) / scale)}
    over = {}
    for k, (e_hip, e_32) in rows.items():
        bar = max(ENVELOPE_K * e_32, ENVELOPE_FLOOR)
        print(f"{what} {k}: hip {e_hip:.2e} fp32 {e_32:.2e} bar {bar:.2e}")
        if not e_hip <= bar:
            over[k] = (e_hip, bar)
    assert not over, (what, over)


def _run(K, H, sigma, kind, grouped):
    B, R, live, ins = 3, 4, 2, 2
    n = B * R if grouped else 5
    src, pos, u8, tgt, w, dout, r64, r32 = _case(K, H, sigma, n, kind, grouped)
    # (the reference, before the kernel) not vacuous
    assert np.abs(r64).max() > 0 and abs(r64.sum()) >= 0.05 * np.abs(r64).sum()
    fr = 3 * H * H
    sdev = torch.tensor([sigma], device=DEV, dtype=torch.float64)
    kw = {}
    if grouped:
        T = R + ins
        pvs = torch.zeros(B, R + 1, 2 * K)
        pvs[:, 1:] = pos.view(B, R, 2 * K)
        x = torch.zeros(B, T, 3, H, H)
        x[:, ins:] = tgt.view(B, R, 3, H, H)
        x[:, ins + live:] = NAN                       # dead steps: poisoned
        x8 = torch.zeros(B, T, 3, H, H, dtype=torch.uint8)
        x8[:, ins:] = u8.view(B, R, 3, H, H)
        pd, xd, x8d = pvs.to(DEV).contiguous(), x.to(DEV).contiguous(), x8.to(DEV).contiguous()
        pv, tv = (p_(pd) + 2 * K * 4, (R + 1) * 2 * K, 2 * K, R), (T * fr, R, fr)
        kw["live"] = live
        t32, t8 = p_(xd) + ins * fr * 4, p_(x8d) + ins * fr
        lw = (2, 0.83, B, 1, R, live)
    else:
        pd, xd, x8d = pos.to(DEV).contiguous(), tgt.to(DEV).contiguous(), u8.to(DEV).contiguous()
        pv, tv = (p_(pd), 0, 2 * K, 0), (fr, 0, 0)
        t32, t8 = p_(xd), p_(x8d)
        lw = (1, 0.37, n, 1, 1, 1)
    if kind == "dsse":
        kw.update(tgt=t32, w=w)
    elif kind == "t8":
        kw.update(tgt8=t8, w=w)
    elif kind == "lw":
        kw.update(tgt=t32, lw=lw)
    else:   # dense: no SSE weight; the target pointer still addresses n valid frames
        dd = dout.to(DEV).contiguous()
        kw.update(tgt=p_(dd), dout=dout)
    what = f"K={K} H={H} sigma={sigma} {kind}{' grouped' if grouped else ''}"
    dpos, slab, dsig = _launch(K, H, src, pv, tv, n, sigma_dev=sdev, **kw)
    assert np.isfinite(dsig).all() and torch.isfinite(dpos).all(), what
    # (i) dsig on / off: the other outputs bit for bit
    dpos0, slab0, none = _launch(K, H, src, pv, tv, n, sigma_dev=sdev, want_dsig=False, **kw)
    assert none is None and torch.equal(dpos, dpos0) and torch.equal(slab, slab0), what + ": dsig changes the outputs"
    # (ii) the existing host-sigma entry point, which runs the same generic kernel below 1
    if sigma < 1.0:
        dposh, slabh, _ = _launch(K, H, src, pv, tv, n, host_sigma=sigma, **kw)
        assert torch.equal(dpos0, dposh) and torch.equal(slab0, slabh), what + ": differs from the host-sigma launch"
    # two launches: the same bits
    again = _launch(K, H, src, pv, tv, n, sigma_dev=sdev, **kw)[2]
    assert np.array_equal(dsig, again), what + ": second launch differs"
    if grouped:
        d = dsig.reshape(B, R)
        assert (d[:, live:] == 0.0).all() and (r64.reshape(B, R)[:, live:] == 0.0).all(), what + ": dead frames"
    # (iii) against float64 autograd
    _judge(dsig, r64, r32, what)


def _cases(kinds):
    """(K, H, kind): byte targets and in-kernel loss weights on the one-CU shapes only."""
    return [(K, H, k) for K, H in SHAPES for k in kinds if k in ("dsse", "dense") or (K, H) in CU_SHAPES]


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("K,H,kind", _cases(["dsse", "lw", "dense", "t8"]))
def test_dsig_ungrouped(K, H, kind, sigma):
    _run(K, H, sigma, kind, False)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("K,H,kind", _cases(["dsse", "lw", "t8"]))
def test_dsig_grouped_live(K, H, kind, sigma):
    _run(K, H, sigma, kind, True)


# ------------------------------------------------------- sigma from u, chain rule
US = [-3.0, -0.5, 0.0, 0.5, 3.0]


def _ulps(a, b, dtype):
    return abs(float(a) - float(b)) / float(np.spacing(np.abs(dtype(b))))


@pytest.mark.parametrize("u", US)
def test_sigma_from_u(u):
    ud = torch.tensor(u, device=DEV)
    sg = torch.full((1,), NAN, device=DEV, dtype=torch.float64)
    L().paig_sigma_from_u(p_(ud), p_(sg), st())
    torch.cuda.synchronize()
    want = np.exp(np.log(2.0) * np.tanh(np.float64(np.float32(u))))
    got = float(sg.cpu()[0])
    print(u, got, want, _ulps(got, want, np.float64))
    assert _ulps(got, want, np.float64) <= 4
    assert 0.5 < got < 2.0
    if u == 0.0:
        assert got == 1.0


@pytest.mark.parametrize("u", US)
def test_sigma_grad_chain_rule_and_accumulate(u):
    g = torch.Generator().manual_seed(3)
    a = torch.rand(301, generator=g, dtype=torch.float64) + 0.5     # no cancellation: the sum's order is immaterial
    b = torch.rand(77, generator=g, dtype=torch.float64) * 3.0
    ad, bd, ud = a.to(DEV), b.to(DEV), torch.tensor(u, device=DEV)
    u64 = np.float64(np.float32(u))
    t = np.tanh(u64)
    dsdu = np.log(2.0) * np.exp(np.log(2.0) * t) * (1.0 - t * t)
    lib = L()
    for name, (x, nx, y, ny, tot) in {"both": (ad, 301, bd, 77, a.sum() + b.sum()),
                                      "first only": (ad, 301, None, 0, a.sum())}.items():
        want = np.float32(float(tot) * dsdu)
        gu = torch.full((), NAN, device=DEV)
        lib.paig_sigma_grad(p_(x), nx, p_(y), ny, p_(ud), p_(gu), 0, st())
        torch.cuda.synchronize()
        got = np.float32(gu.cpu().item())
        assert _ulps(got, want, np.float32) <= 2, (name, got, want)
        # accumulate onto a non-zero slot; and twice the same bits
        slot = torch.tensor(0.75, device=DEV)
        lib.paig_sigma_grad(p_(x), nx, p_(y), ny, p_(ud), p_(slot), 1, st())
        gu2 = torch.full((), NAN, device=DEV)
        lib.paig_sigma_grad(p_(x), nx, p_(y), ny, p_(ud), p_(gu2), 0, st())
        torch.cuda.synchronize()
        assert np.float32(slot.cpu().item()) == np.float32(np.float32(0.75) + got), name
        assert gu2.cpu().item() == gu.cpu().item(), name
