"""The decoder kernels' sigma entry points (paig_decoder_*_sigma) against
autograd through the oracle's decoder restated with the attention-window scale
(tests/sigma_ref.py; reference physics_models.py:160-182), on the CPU in fp32.
Mirrors test_gpu_decoder.py at the smallest instantiated shapes, for sigma in
{0.5, 0.7} (the one-CU shapes' backward takes the generic kernels: a source
texel gathers up to 9 output indices per axis) and {1.5, 2.0} (the one-CU
kernels, 5-wide tables):

  * an ungrouped ragged count (F = 5), loss weights from an array and formed
    in-kernel (lw_mode 1), float and uint8 targets, two launches bit-identical;
  * grouped frames B = 3, R = 4, live = 2 (dead steps' targets NaN, their
    position gradients 0), weights from an array and in-kernel (lw_mode 2);
  * a dense dL/dout without an SSE weight;
  * the forward's frames and fused SSE (float and uint8 targets);
  * paig_decoder_parts_sigma;
  * the old entry points against the new ones at sigma = 1.0, bit for bit;
  * paig_decoder_fwd_rollout_sigma against the unfused launches, bit for bit.

Bar: 1e-4 normwise.  The bilinear derivative jumps where a sampling coordinate
crosses an integer (at sigma = 2 every pixel of a frame shares one fractional
offset), so each case's positions come from the first seed for which no
sampling coordinate of the CPU reference lies within 1e-3 px of an integer;
the test asserts that property of the positions it uses."""
import functools
import types

import pytest
import torch

from helpers import rel_err
import sigma_ref as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(2, 32), (3, 36), (2, 64)]
SIGMAS = [0.5, 0.7, 1.5, 2.0]
BAR = 1e-4
NAN = float("nan")


def L():
    from paig_reproduction_amd._lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def p_(t):
    return None if t is None else t.data_ptr()


def _sources(K, H, seed):
    g = torch.Generator().manual_seed(seed)
    h = H // 2
    tmpl = torch.randn(K, 1, h, h, generator=g) * 2.0
    cont = torch.randn(K, 3, h, h, generator=g)
    bg = torch.sigmoid(torch.randn(1, 3, H, H, generator=g))
    return tmpl, cont, bg


def _tie_distance(K, H, pos, sigma):
    c = SR.sample_coords(K, H, pos, SR.sigma_of(sigma))
    return (c - torch.round(c)).abs().min().item()


@functools.lru_cache(maxsize=None)
def _positions(n, K, H, sigma, seed0):
    """test_gpu_decoder.py's generator ((rand*1.5 - 0.25)*H: windows partly and
    wholly outside the frame), first seed >= seed0 without a near tie."""
    for seed in range(seed0, seed0 + 4000):
        g = torch.Generator().manual_seed(seed)
        pos = (torch.rand(n, 2 * K, generator=g) * 1.5 - 0.25) * H
        if _tie_distance(K, H, pos, sigma) > 1e-3:
            return pos
    raise AssertionError("no tie-free seed")


def _cfg(K, H):
    return types.SimpleNamespace(n_objs=K, tmpl=H // 2, size=H)


def _reference(K, H, sigma, tmpl, cont, bg, pos, tgt, w, dout):
    """Autograd of sum_f w_f ||out_f - tgt_f||^2 + <dout, out> (fp32, CPU)."""
    assert _tie_distance(K, H, pos, sigma) > 1e-3
    t = tmpl.clone().requires_grad_(True)
    sc = torch.sigmoid(cont).requires_grad_(True)
    b = bg.clone().requires_grad_(True)
    p = pos.clone().requires_grad_(True)
    joint = torch.cat([t.repeat(1, 3, 1, 1) + 5, sc], 1)
    out = SR.st_decoder_sigma(_cfg(K, H), joint, b, p, SR.sigma_of(sigma))
    loss = 0.0
    if w is not None:
        loss = loss + (w.view(-1, 1, 1, 1) * (out - tgt) ** 2).sum()
    if dout is not None:
        loss = loss + (out * dout).sum()
    loss.backward()
    return p.grad, t.grad.reshape(-1), sc.grad.reshape(-1), b.grad.reshape(-1)


def _bwd(K, H, sigma, src, pos_view, tgt=None, tgt8=None, tgt_view=(0, 0, 0), w=None, lw=None, dout=None, F_=0,
         live=0, old=False, raw=False):
    """paig_decoder_bwd_ex_sigma (old: paig_decoder_bwd_ex) + the slab
    reduction: (dpos, d template, d sigmoid(content), d background)."""
    h = H // 2
    lib = L()
    td, cd, bd = (s.to(DEV).contiguous() for s in src)
    slab_len = int(lib.paig_decoder_slab_len(K, h, H))
    grp = pos_view[3]
    if old:
        nb, scr_n = lib.paig_decoder_bwd_blocks(F_, grp, live, K, h, H), lib.paig_decoder_bwd_scratch(F_, K, h, H)
    else:
        nb = lib.paig_decoder_bwd_blocks_sigma(F_, grp, live, K, h, H, sigma)
        scr_n = lib.paig_decoder_bwd_scratch_sigma(F_, K, h, H, sigma)
    slab = torch.full((nb * slab_len,), NAN, device=DEV)
    scratch = torch.empty(scr_n, device=DEV) if scr_n else None
    dpos = torch.full((F_, 2 * K), NAN, device=DEV)
    wd = w.to(DEV) if w is not None else None
    dd = dout.to(DEV).contiguous() if dout is not None else None
    keep = []
    if lw is not None:   # (mode, dt, B, Te, R, pred): in-kernel weights from the train-loss adjoint alone
        mode, dtv, lB, lTe, lR, lpred = lw
        dtd = torch.tensor([dtv], device=DEV)
        keep.append(dtd)
        lwa = (mode, p_(dtd), None, None, 0.0, lB, lTe, lR, lpred)
    else:
        lwa = (0, None, None, None, 0.0, 0, 0, 0, 0)
    args = (*pos_view, p_(td), p_(cd), p_(bd), tgt, tgt8, None, *tgt_view, p_(wd), *lwa, p_(dd), 3 * H * H, p_(dpos),
            p_(slab), p_(scratch), F_, live, K, h, H)
    if old:
        lib.paig_decoder_bwd_ex(*args, st())
    else:
        lib.paig_decoder_bwd_ex_sigma(*args, sigma, st())
    dsrc = torch.empty(slab_len, device=DEV)
    lib.paig_slab_reduce(p_(slab), nb, slab_len, slab_len, p_(dsrc), 0, st())
    torch.cuda.synchronize()
    if raw:
        return dpos.cpu(), slab.cpu()
    ds = dsrc.cpu()
    return dpos.cpu(), ds[:K * h * h], ds[K * h * h:4 * K * h * h], ds[4 * K * h * h:]


def _check(got, ref, what):
    for a, b, n in zip(got, ref, ("dpos", "d_template", "d_content", "d_background")):
        e = rel_err(a, b)
        assert e <= BAR, f"{what}: {n} rel err {e:.3g}"


def _same(a, b, what):
    for x, y, n in zip(a, b, ("dpos", "d_template", "d_content", "d_background")):
        assert torch.equal(x, y), f"{what}: {n} differs"


def _u8_targets(n, H, seed):
    u8 = torch.randint(0, 256, (n, 3, H, H), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return u8, u8.float() / 255.0


@pytest.mark.parametrize("K,H", SHAPES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_bwd_ungrouped(K, H, sigma):
    F_ = 5
    src = _sources(K, H, 10 * K + H)
    pos = _positions(F_, K, H, sigma, 1)
    u8, tgt = _u8_targets(F_, H, 99)
    w = torch.rand(F_, generator=torch.Generator().manual_seed(7)) + 0.1
    ref = _reference(K, H, sigma, *src, pos, tgt, w, None)
    pd, td, ud = pos.to(DEV).contiguous(), tgt.to(DEV).contiguous(), u8.to(DEV).contiguous()
    pv, fr = (p_(pd), 0, 2 * K, 0), 3 * H * H
    what = f"K={K} H={H} sigma={sigma}"
    a = _bwd(K, H, sigma, src, pv, tgt=p_(td), tgt_view=(fr, 0, 0), w=w, F_=F_)
    _check(a, ref, what)
    _same(a, _bwd(K, H, sigma, src, pv, tgt=p_(td), tgt_view=(fr, 0, 0), w=w, F_=F_), what + " second launch")
    _same(a, _bwd(K, H, sigma, src, pv, tgt8=p_(ud), tgt_view=(fr, 0, 0), w=w, F_=F_), what + " uint8 targets")
    # in-kernel weights, lw_mode 1 (reconstruction frames): dr / (B Te) on every frame
    dr = 0.37
    refl = _reference(K, H, sigma, *src, pos, tgt, torch.full((F_,), dr / F_), None)
    drd = torch.tensor([dr], device=DEV)
    got = _bwd_lw1(K, H, sigma, src, pv, p_(td), None, fr, drd, F_)
    _check(got, refl, what + " lw_mode 1")
    _same(got, _bwd_lw1(K, H, sigma, src, pv, None, p_(ud), fr, drd, F_), what + " lw_mode 1 uint8")


def _bwd_lw1(K, H, sigma, src, pv, tgt, tgt8, fr, drd, F_):
    """lw_mode 1 (reconstruction frames): weight dr / (B Te), B Te = F."""
    h = H // 2
    lib = L()
    td, cd, bd = (s.to(DEV).contiguous() for s in src)
    slab_len = int(lib.paig_decoder_slab_len(K, h, H))
    nb = lib.paig_decoder_bwd_blocks_sigma(F_, 0, 0, K, h, H, sigma)
    scr_n = lib.paig_decoder_bwd_scratch_sigma(F_, K, h, H, sigma)
    slab = torch.full((nb * slab_len,), NAN, device=DEV)
    scratch = torch.empty(scr_n, device=DEV) if scr_n else None
    dpos = torch.full((F_, 2 * K), NAN, device=DEV)
    lib.paig_decoder_bwd_ex_sigma(*pv, p_(td), p_(cd), p_(bd), tgt, tgt8, None, fr, 0, 0, None, 1, None, None, p_(drd),
                                  0.0, F_, 1, 1, 1, None, 3 * H * H, p_(dpos), p_(slab), p_(scratch), F_, 0, K, h, H,
                                  sigma, st())
    dsrc = torch.empty(slab_len, device=DEV)
    lib.paig_slab_reduce(p_(slab), nb, slab_len, slab_len, p_(dsrc), 0, st())
    torch.cuda.synchronize()
    ds = dsrc.cpu()
    return dpos.cpu(), ds[:K * h * h], ds[K * h * h:4 * K * h * h], ds[4 * K * h * h:]


@pytest.mark.parametrize("K,H", SHAPES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_bwd_live_steps(K, H, sigma):
    """The rollout layout: positions pvs[B][R+1][2K] from step 1, targets
    input[B][T][3][H][W] from frame ins; steps >= live are dead (NaN targets)."""
    B, R, live, ins = 3, 4, 2, 2
    T = R + ins
    src = _sources(K, H, 7 * K + H + R)
    pvs = torch.zeros(B, R + 1, 2 * K)
    pvs[:, 1:] = _positions(B * R, K, H, sigma, 50).view(B, R, 2 * K)
    u8, xf = _u8_targets(B * T, H, 5)
    x = xf.view(B, T, 3, H, H).clone()
    x[:, ins + live:] = NAN
    g = torch.Generator().manual_seed(B * 100 + R)
    w = torch.zeros(B, R)
    w[:, :live] = torch.rand(B, live, generator=g) + 0.1
    pd, xd, ud = pvs.to(DEV).contiguous(), x.to(DEV).contiguous(), u8.to(DEV).contiguous()
    fr = 3 * H * H
    pv = (p_(pd) + 2 * K * 4, (R + 1) * 2 * K, 2 * K, R)
    pos = pvs[:, 1:].reshape(B * R, 2 * K)
    tgt = torch.nan_to_num(x[:, ins:].reshape(B * R, 3, H, H), nan=0.0)
    what = f"K={K} H={H} sigma={sigma} live"
    got = _bwd(K, H, sigma, src, pv, tgt=p_(xd) + ins * fr * 4, tgt_view=(T * fr, R, fr), w=w.reshape(-1), F_=B * R,
               live=live)
    assert torch.isfinite(got[0]).all(), "dead-step position gradients not written"
    assert (got[0].view(B, R, 2 * K)[:, live:] == 0).all()
    _check(got, _reference(K, H, sigma, *src, pos, tgt, w.reshape(-1), None), what)
    g8 = _bwd(K, H, sigma, src, pv, tgt8=p_(ud) + ins * fr, tgt_view=(T * fr, R, fr), w=w.reshape(-1), F_=B * R,
              live=live)
    _same(got, g8, what + " uint8 targets")
    # in-kernel weights (lw_mode 2): dt / (B pred) on the pred = live steps, none beyond (no extrap adjoint)
    dt = 0.83
    wl = torch.zeros(B, R)
    wl[:, :live] = dt / (B * live)
    refl = _reference(K, H, sigma, *src, pos, tgt, wl.reshape(-1), None)
    for kw, tag in ((dict(tgt=p_(xd) + ins * fr * 4), "float"), (dict(tgt8=p_(ud) + ins * fr), "uint8")):
        gl = _bwd(K, H, sigma, src, pv, tgt_view=(T * fr, R, fr), lw=(2, dt, B, 1, R, live), F_=B * R, live=live, **kw)
        assert (gl[0].view(B, R, 2 * K)[:, live:] == 0).all()
        _check(gl, refl, what + " lw_mode 2 " + tag)


@pytest.mark.parametrize("K,H", SHAPES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_bwd_dense(K, H, sigma):
    F_ = 5
    src = _sources(K, H, 3 * K + H)
    pos = _positions(F_, K, H, sigma, 200)
    dout = torch.randn(F_, 3, H, H, generator=torch.Generator().manual_seed(4))
    pd, dd = pos.to(DEV).contiguous(), dout.to(DEV).contiguous()
    got = _bwd(K, H, sigma, src, (p_(pd), 0, 2 * K, 0), tgt=p_(dd), tgt_view=(3 * H * H, 0, 0), dout=dout, F_=F_)
    _check(got, _reference(K, H, sigma, *src, pos, None, None, dout), f"dense K={K} H={H} sigma={sigma}")


def _fwd(K, H, sigma, src, pv, F_, tgt=None, tgt8=None, tgt_view=(0, 0, 0), old=False):
    lib = L()
    td, cd, bd = (s.to(DEV).contiguous() for s in src)
    fr = 3 * H * H
    out = torch.full((F_, 3, H, H), NAN, device=DEV)
    sse = torch.full((F_,), NAN, device=DEV)
    head = (*pv, p_(td), p_(cd), p_(bd), p_(out), fr)
    tail = (p_(sse) if (tgt or tgt8) else None, F_, K, H // 2, H)
    fs, grp, gs = tgt_view
    if tgt8:
        (lib.paig_decoder_fwd_t8 if old else lib.paig_decoder_fwd_t8_sigma)(
            *head, tgt8, None, fs, grp, gs, *tail, *(() if old else (sigma,)), st())
    else:
        (lib.paig_decoder_fwd if old else lib.paig_decoder_fwd_sigma)(
            *head, tgt, fs, grp, gs, *tail, *(() if old else (sigma,)), st())
    torch.cuda.synchronize()
    return out.cpu(), sse.cpu()


@pytest.mark.parametrize("K,H", SHAPES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_fwd_frames_sse_and_parts(K, H, sigma):
    F_ = 5
    src = _sources(K, H, 5 * K + H)
    tmpl, cont, bg = src
    pos = _positions(F_, K, H, sigma, 300)
    u8, tgt = _u8_targets(F_, H, 11)
    pd, td, ud = pos.to(DEV).contiguous(), tgt.to(DEV).contiguous(), u8.to(DEV).contiguous()
    pv, fr = (p_(pd), 0, 2 * K, 0), 3 * H * H
    joint = torch.cat([tmpl.repeat(1, 3, 1, 1) + 5, torch.sigmoid(cont)], 1)
    s = SR.sigma_of(sigma)
    ro = SR.st_decoder_sigma(_cfg(K, H), joint, bg, pos, s)
    rs = ((ro - tgt) ** 2).sum((1, 2, 3))
    out, sse = _fwd(K, H, sigma, src, pv, F_, tgt=p_(td), tgt_view=(fr, 0, 0))
    assert rel_err(out, ro) <= BAR and rel_err(sse, rs) <= BAR
    o8, s8 = _fwd(K, H, sigma, src, pv, F_, tgt8=p_(ud), tgt_view=(fr, 0, 0))
    assert torch.equal(o8, out) and torch.equal(s8, sse)
    o2, s2 = _fwd(K, H, sigma, src, pv, F_, tgt=p_(td), tgt_view=(fr, 0, 0))
    assert torch.equal(o2, out) and torch.equal(s2, sse)
    # the per-object intermediates
    cd_, md_ = (torch.full((K + 1, F_, 3, H, H), NAN, device=DEV) for _ in range(2))
    tdev, cdev, bdev = (t.to(DEV).contiguous() for t in src)
    L().paig_decoder_parts_sigma(p_(pd), 2 * K, p_(tdev), p_(cdev), p_(bdev), p_(cd_), p_(md_), F_, K, H // 2, H, sigma,
                                 st())
    torch.cuda.synchronize()
    rc, rm = SR.st_decoder_parts_sigma(_cfg(K, H), joint, bg, pos, s)
    for k in range(K + 1):
        assert rel_err(cd_[k], rc[k]) <= BAR, f"content {k}"
        assert rel_err(md_[k], rm[k]) <= BAR, f"mask {k}"


@pytest.mark.parametrize("K,H", SHAPES)
def test_old_entry_points_are_sigma_one(K, H):
    """Frames, SSE, dpos and the slab rows: bit-identical."""
    F_ = 7
    src = _sources(K, H, K + H)
    pos = _positions(F_, K, H, 1.0, 400)
    u8, tgt = _u8_targets(F_, H, 3)
    w = torch.rand(F_, generator=torch.Generator().manual_seed(2)) + 0.1
    pd, td, ud = pos.to(DEV).contiguous(), tgt.to(DEV).contiguous(), u8.to(DEV).contiguous()
    pv, fr = (p_(pd), 0, 2 * K, 0), 3 * H * H
    for kw in (dict(tgt=p_(td)), dict(tgt8=p_(ud))):
        a = _fwd(K, H, 1.0, src, pv, F_, tgt_view=(fr, 0, 0), old=True, **kw)
        b = _fwd(K, H, 1.0, src, pv, F_, tgt_view=(fr, 0, 0), **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a = _bwd(K, H, 1.0, src, pv, tgt_view=(fr, 0, 0), w=w, F_=F_, old=True, raw=True, **kw)
        b = _bwd(K, H, 1.0, src, pv, tgt_view=(fr, 0, 0), w=w, F_=F_, raw=True, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    lib = L()
    assert lib.paig_decoder_bwd_blocks(F_, 0, 0, K, H // 2, H) == lib.paig_decoder_bwd_blocks_sigma(F_, 0, 0, K, H // 2,
                                                                                                   H, 1.0)


def test_sigma_out_of_range_is_an_error():
    from paig_reproduction_amd._lib import PaigError
    K, H, F_ = 2, 32, 2
    src = _sources(K, H, 1)
    pd = _positions(F_, K, H, 1.0, 400).to(DEV).contiguous()
    for bad in (0.49, 2.01, 4.0, NAN):
        with pytest.raises(PaigError, match="sigma"):
            _fwd(K, H, bad, src, (p_(pd), 0, 2 * K, 0), F_)


# ---------------------------------------------------------------- fused rollout + decode
@pytest.mark.parametrize("K,H,cell,sigma", [(2, 32, 0, 2.0), (2, 32, 1, 0.5), (3, 36, 2, 1.5), (2, 64, 0, 0.7)])
def test_fused_rollout_decode_matches_parts(K, H, cell, sigma):
    """paig_decoder_fwd_rollout_sigma = paig_rollout_fwd + paig_decoder_fwd_sigma, bit for bit."""
    B, R, Te, D = 3, 4, 2, 2 * K
    lib = L()
    g = torch.Generator().manual_seed(17 + cell)
    src = _sources(K, H, 31)
    td, cd, bd = (s.to(DEV).contiguous() for s in src)
    F_ = B * Te
    pos = _positions(F_, K, H, sigma, 500).to(DEV).contiguous()
    x = torch.rand(F_, 3, H, H, generator=g).to(DEV)
    pos0 = (torch.rand(B, D, generator=g) * 0.5 + 0.25).mul(H).to(DEV)
    vel0 = (torch.randn(B, D, generator=g)).to(DEV)
    dt = torch.tensor([0.3], device=DEV)
    q = torch.tensor([0.7, 1.1], device=DEV, dtype=torch.float64)
    fr = 3 * H * H

    def run(fused):
        pvs = torch.zeros((B, R + 1, 2 * D), device=DEV)
        out = torch.full((F_, 3, H, H), NAN, device=DEV)
        sse = torch.full((F_,), NAN, device=DEV)
        roll = (cell, p_(pos0), D, p_(vel0), p_(dt), p_(q), p_(q) + 8, p_(pvs), B, D, R)
        dec = (p_(pos), 0, 2 * K, 0, p_(td), p_(cd), p_(bd), p_(out), fr, p_(x), fr, 0, 0, p_(sse), F_, K, H // 2, H,
               sigma)
        if fused:
            lib.paig_decoder_fwd_rollout_sigma(*roll, *dec, st())
        else:
            lib.paig_rollout_fwd(*roll, st())
            lib.paig_decoder_fwd_sigma(*dec, st())
        torch.cuda.synchronize()
        return pvs.cpu(), out.cpu(), sse.cpu()

    a, b = run(True), run(False)
    for u, v, n in zip(a, b, ("pvs", "frames", "sse")):
        assert torch.isfinite(u).all(), n
        assert torch.equal(u, v), n
