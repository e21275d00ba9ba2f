"""The loss kernels and the decoder backward's in-kernel loss weights, called
directly (the training step only ever drives them with train_loss's adjoint):

  paig_loss_reduce     per-frame SSE -> (train, extrap, recons), against
                       float64 numpy of the reference's compute_loss
                       (nn/network/physics_models.py:119-142);
  paig_loss_bwd        loss adjoints (dt, de, dr; any may be null) -> the
                       per-frame weights dL/dSSE, against float64 numpy of
                       loss_weight (csrc/common.h);
  paig_decoder_bwd_ex  lw_mode 1 (reconstruction frames, ungrouped) and 2
                       (rollout frames grouped by R): the weights formed in
                       the kernel from the adjoints.  Bit-identical to the
                       same entry point reading the arrays paig_loss_bwd wrote
                       (lw_mode 0), and within the decoder tests' 1e-4 of
                       autograd through the oracle's decoder with the weights
                       formed on the host in float64.

Bars: 1e-5 for the reduction (the single-op bar of test_gpu_kernels.py);
1e-6 for the weights (each is at most three fp32 roundings of same-sign
terms: the product ae * dt, the sum, the division: ~2e-7); 1e-4 normwise
for the decoder gradients (test_gpu_decoder.py)."""
import functools

import numpy as np
import pytest
import torch

from helpers import rel_err
from test_gpu_decoder import DEV, SHAPES, L, _positions, _reference, _sources

pytestmark = pytest.mark.gpu

ADJ = {"dt": 0.7, "de": 1.3, "dr": 2.1}
LOSS_SHAPES = [(1, 1, 1, 1), (3, 5, 7, 4), (37, 10, 46, 6), (2, 4, 4, 4)]   # (B, Te, R, pred)
SUBSETS = [("dt",), ("de",), ("dr",), ("dt", "de"), ("dt", "dr"), ("de", "dr"), ("dt", "de", "dr")]
DEC_DIMS = [(3, 5, 7, 4), (2, 4, 4, 4), (5, 3, 9, 1)]
DEC_SETS = [(("dt",), 2.0), (("de",), 2.0), (("dr",), 2.0), (("dt", "de"), 2.0), (("dt", "dr"), 2.0),
            (("dt", "de", "dr"), 2.0), (("dt",), 0.0), (("dt", "dr"), 0.0)]
INS = 2


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _adjoints(names, sign=1.0):
    """{name: 0-dim fp32 device tensor} and the same values in float64."""
    dev = {k: torch.tensor(sign * ADJ[k], dtype=torch.float32, device=DEV) for k in names}
    host = {k: float(np.float64(np.float32(sign * ADJ[k]))) for k in names}
    return dev, host


def _host_weights(adj, ae, B, Te, R, pred):
    """loss_weight (csrc/common.h) for every frame, float64: (wrec [B*Te],
    wroll [B*R]).  dt is the adjoint of train = pred + ae * recons (Q2)."""
    dt, de, dr = (adj.get(k, 0.0) for k in ("dt", "de", "dr"))
    wroll = np.zeros((B, R))
    wroll[:, :pred] = dt / (B * pred)
    if R > pred:
        wroll[:, pred:] = de / (B * (R - pred))
    wrec = np.full(B * Te, ((ae * dt if ae > 0 else 0.0) + dr) / (B * Te))
    return wrec, wroll.reshape(-1)


def _loss_bwd(adj_dev, ae, B, Te, R, pred):
    wrec = torch.full((B * Te,), float("nan"), device=DEV)
    wroll = torch.full((B * R,), float("nan"), device=DEV)
    L().paig_loss_bwd(_p(adj_dev.get("dt")), _p(adj_dev.get("de")), _p(adj_dev.get("dr")), ae, _p(wrec), _p(wroll),
                      B, Te, R, pred, _st())
    torch.cuda.synchronize()
    return wrec, wroll


# ------------------------------------------------------------ loss_reduce
@pytest.mark.parametrize("ae", [0.0, 2.0])
@pytest.mark.parametrize("B,Te,R,pred", LOSS_SHAPES)
def test_loss_reduce(B, Te, R, pred, ae):
    g = torch.Generator().manual_seed(B * 1000 + R)
    sse_rec = torch.rand(B * Te, generator=g) * 50
    sse_roll = torch.rand(B * R, generator=g) * 80
    out = torch.full((3,), float("nan"), device=DEV)
    a, b = sse_rec.to(DEV), sse_roll.to(DEV)
    L().paig_loss_reduce(_p(a), _p(b), B, Te, R, pred, ae, out.data_ptr(), out.data_ptr() + 4, out.data_ptr() + 8,
                         _st())
    torch.cuda.synchronize()
    train, extrap, recons = out.double().cpu().numpy()
    roll = sse_roll.double().numpy().reshape(B, R)
    r_pred = roll[:, :pred].mean()
    r_rec = sse_rec.double().numpy().mean()
    r_train = r_pred + ae * r_rec if ae > 0 else r_pred
    assert rel_err(np.float64(train), np.float64(r_train)) <= 1e-5, (train, r_train)
    assert rel_err(np.float64(recons), np.float64(r_rec)) <= 1e-5, (recons, r_rec)
    if R == pred:
        # no extrapolation steps: the mean of an empty slice, as torch's
        assert np.isnan(extrap) and np.isfinite(train) and np.isfinite(recons)
    else:
        r_ext = roll[:, pred:].mean()
        assert rel_err(np.float64(extrap), np.float64(r_ext)) <= 1e-5, (extrap, r_ext)


# --------------------------------------------------------------- loss_bwd
@pytest.mark.parametrize("ae", [0.0, 2.0])
@pytest.mark.parametrize("B,Te,R,pred", LOSS_SHAPES)
def test_loss_bwd(B, Te, R, pred, ae):
    got = {}
    for names, sign in [(s, 1.0) for s in SUBSETS] + [(("dt", "de", "dr"), -1.0)]:
        adj_dev, adj = _adjoints(names, sign)
        wrec, wroll = _loss_bwd(adj_dev, ae, B, Te, R, pred)
        what = f"{names} sign {sign}"
        assert torch.isfinite(wrec).all() and torch.isfinite(wroll).all(), f"{what}: an element was not written"
        r_rec, r_roll = _host_weights(adj, ae, B, Te, R, pred)
        e_rec, e_roll = rel_err(wrec, r_rec), rel_err(wroll, r_roll)
        print(f"loss_bwd {B, Te, R, pred} ae={ae} {what}: rec {e_rec:.2e} roll {e_roll:.2e}")
        assert e_rec <= 1e-6, (what, e_rec)
        assert e_roll <= 1e-6, (what, e_roll)
        # a weight whose every term is absent is exactly zero
        assert (wrec == 0).all() == (not np.any(r_rec)), what
        assert torch.equal(wroll == 0, torch.from_numpy(r_roll == 0).to(DEV)), what
        got[(names, sign)] = wroll
    if R == pred:
        # no extrapolation steps: the de term contributes exactly nothing
        assert (got[(("de",), 1.0)] == 0).all()
        assert torch.equal(got[(("dt", "de"), 1.0)], got[(("dt",), 1.0)])
        assert torch.equal(got[(("dt", "de", "dr"), 1.0)], got[(("dt", "dr"), 1.0)])


# ------------------------------------------------- decoder backward, lw modes
def _unit_refs(K, H, tmpl, cont, bg, pos, tgt, classes):
    """Autograd gradients (fp32, CPU) for unit weights on each frame class,
    as float64: the loss is linear in the weights, so any weighting's
    reference is a float64 combination of these."""
    return [tuple(t.double() for t in _reference(K, H, tmpl, cont, bg, pos, tgt, c.float(), None)) for c in classes]


@functools.lru_cache(maxsize=None)
def _case(K, H, B, Te, R, pred, mode):
    """One decoder problem: sources, positions, targets (bytes / 255, so the
    byte-target kernels see the same frames) and the unit-weight references."""
    tmpl, cont, bg = _sources(K, H, 13 * K + H + R)
    g = torch.Generator().manual_seed(B * 100 + R + mode)
    fr = 3 * H * H
    c = {"K": K, "H": H, "src": [t.to(DEV).contiguous() for t in (tmpl, cont, bg)], "fr": fr}
    if mode == 1:
        F_ = B * Te
        pos = _positions(F_, K, H, F_ + 1)
        tgt = torch.randint(0, 256, (F_, 3, H, H), generator=g, dtype=torch.uint8).float() / 255
        c.update(F=F_, pos_t=pos.to(DEV).contiguous(), tgt_t=tgt.to(DEV).contiguous())
        c["pos_view"] = (c["pos_t"].data_ptr(), 0, 2 * K, 0)
        c["tgt_view"] = (c["tgt_t"].data_ptr(), fr, 0, 0)
        classes = [torch.ones(F_)]
    else:
        T, N = R + INS, B + 2
        pvs = torch.zeros(B, R + 1, 2 * K)
        pvs[:, 1:] = _positions(B * R, K, H, B + R).view(B, R, 2 * K)
        u8 = torch.randint(0, 256, (N, T, 3, H, H), generator=g, dtype=torch.uint8)
        rows = torch.randperm(N, generator=g)[:B]
        x = u8[rows].float() / 255
        xp = x.clone()
        xp[:, INS + pred:] = float("nan")   # the frames a live = pred launch must never read
        pos, tgt = pvs[:, 1:].reshape(B * R, 2 * K), x[:, INS:].reshape(B * R, 3, H, H)
        c.update(F=B * R, pos_t=pvs.to(DEV).contiguous(), tgt_t=x.to(DEV).contiguous(),
                 tgt_poison=xp.to(DEV).contiguous(), u8=u8.to(DEV).contiguous(), rows=rows.to(DEV).contiguous())
        c["pos_view"] = (c["pos_t"].data_ptr() + 2 * K * 4, (R + 1) * 2 * K, 2 * K, R)
        c["tgt_view"] = (c["tgt_t"].data_ptr() + INS * fr * 4, T * fr, R, fr)
        c["tgt_view_poison"] = (c["tgt_poison"].data_ptr() + INS * fr * 4, T * fr, R, fr)
        # bytes: the dataset's rows through the index, element (= byte) strides
        c["tgt8_view"] = (c["u8"].data_ptr() + INS * fr, c["rows"].data_ptr(), T * fr, R, fr)
        step = torch.arange(B * R) % R
        classes = [(step < pred)] + ([(step >= pred)] if R > pred else [])
    c["refs"] = _unit_refs(K, H, tmpl, cont, bg, pos, tgt, classes)
    return c


def _bwd_ex(c, lw_mode, adj_dev, ae, dims, dsse=None, live=0, tgt="tgt_view", raw=False):
    """paig_decoder_bwd_ex + the slab reduction: (dpos [F, 2K], dsrc), on the
    device.  raw: the unchecked C entry point's return code instead."""
    K, H = c["K"], c["H"]
    h = H // 2
    lib = L()
    F_ = c["F"]
    pv = c["pos_view"]
    slab_len = int(lib.paig_decoder_slab_len(K, h, H))
    nb = lib.paig_decoder_bwd_blocks(F_, pv[3], live, K, h, H)
    slab = torch.full((nb * slab_len,), float("nan"), device=DEV)
    scr_n = lib.paig_decoder_bwd_scratch(F_, K, h, H)
    scratch = torch.empty(scr_n, device=DEV) if scr_n else None
    dpos = torch.full((F_, 2 * K), float("nan"), device=DEV)
    if tgt == "tgt8_view":
        t8, ti, fs, grp, gs = c[tgt]
        tf = None
    else:
        tf, fs, grp, gs = c[tgt]
        t8 = ti = None
    adj_dev = adj_dev or {}
    B, Te, R, pred = dims
    fn = lib.fns["paig_decoder_bwd_ex"] if raw else lib.paig_decoder_bwd_ex
    rc = fn(pv[0], pv[1], pv[2], pv[3], *[t.data_ptr() for t in c["src"]], tf, t8, ti, fs, grp, gs, _p(dsse), lw_mode,
            _p(adj_dev.get("dt")), _p(adj_dev.get("de")), _p(adj_dev.get("dr")), ae, B, Te, R, pred, None, c["fr"],
            dpos.data_ptr(), slab.data_ptr(), _p(scratch), F_, live, K, h, H, _st())
    if raw:
        torch.cuda.synchronize()
        return rc
    dsrc = torch.empty(slab_len, device=DEV)
    lib.paig_slab_reduce(slab.data_ptr(), nb, slab_len, slab_len, dsrc.data_ptr(), 0, _st())
    torch.cuda.synchronize()
    return dpos, dsrc


def _split(c, dpos, dsrc):
    n = c["K"] * (c["H"] // 2) ** 2
    return dpos.cpu(), dsrc[:n].cpu(), dsrc[n:4 * n].cpu(), dsrc[4 * n:].cpu()


def _combine(c, ws):
    """sum_c w_c * (unit reference c), float64."""
    assert len(ws) == len(c["refs"])
    return tuple(sum(float(w) * r[i] for w, r in zip(ws, c["refs"])) for i in range(4))


def _check_ref(c, got, ws, what):
    for a, b, n in zip(_split(c, *got), _combine(c, ws), ("dpos", "d_template", "d_content", "d_background")):
        e = rel_err(a, b.reshape(a.shape))
        assert e <= 1e-4, f"{what}: {n} rel err {e:.3g}"


@pytest.mark.parametrize("B,Te,R,pred", DEC_DIMS)
@pytest.mark.parametrize("K,H", SHAPES)
def test_decoder_bwd_lw_mode1(K, H, B, Te, R, pred):
    """Reconstruction frames (F = B*Te, ungrouped): every frame's weight is
    (ae * dt + dr) / (B * Te)."""
    c = _case(K, H, B, Te, R, pred, 1)
    dims = (B, Te, R, pred)
    for names, ae in DEC_SETS:
        what = f"mode 1 K={K} H={H} {dims} {names} ae={ae}"
        adj_dev, adj = _adjoints(names)
        got = _bwd_ex(c, 1, adj_dev, ae, dims)
        wrec, _ = _loss_bwd(adj_dev, ae, *dims)
        arr = _bwd_ex(c, 0, None, 0.0, (0, 0, 0, 0), dsse=wrec)
        assert torch.equal(got[0], arr[0]), f"{what}: dpos differs from the lw_mode 0 run"
        assert torch.equal(got[1], arr[1]), f"{what}: source gradients differ from the lw_mode 0 run"
        w = _host_weights(adj, ae, *dims)[0][0]
        _check_ref(c, got, [w], what)
        # guard against passing on dead values
        assert bool((got[0] != 0).any()) == (w != 0), what


@pytest.mark.parametrize("B,Te,R,pred", DEC_DIMS)
@pytest.mark.parametrize("K,H", SHAPES)
def test_decoder_bwd_lw_mode2(K, H, B, Te, R, pred):
    """Rollout frames in the engine's layout (grouped by R): the first pred
    steps weigh dt / (B pred), the others de / (B (R - pred)).  Without an
    extrapolation adjoint the launch gets live = pred and NaN in the dead
    targets; their position gradients must be exactly 0."""
    c = _case(K, H, B, Te, R, pred, 2)
    dims = (B, Te, R, pred)
    for names, ae in DEC_SETS:
        what = f"mode 2 K={K} H={H} {dims} {names} ae={ae}"
        adj_dev, adj = _adjoints(names)
        skip_dead = "de" not in names and pred < R
        live, tgt = (pred, "tgt_view_poison") if skip_dead else (0, "tgt_view")
        got = _bwd_ex(c, 2, adj_dev, ae, dims, live=live, tgt=tgt)
        _, wroll = _loss_bwd(adj_dev, ae, *dims)
        arr = _bwd_ex(c, 0, None, 0.0, (0, 0, 0, 0), dsse=wroll, live=live, tgt=tgt)
        assert torch.equal(got[0], arr[0]), f"{what}: dpos differs from the lw_mode 0 run"
        assert torch.equal(got[1], arr[1]), f"{what}: source gradients differ from the lw_mode 0 run"
        w = _host_weights(adj, ae, *dims)[1]
        ws = [w[0]] + ([w[pred]] if R > pred else [])
        _check_ref(c, got, ws, what)
        dpos = got[0].view(B, R, 2 * K)
        assert torch.isfinite(dpos).all(), f"{what}: position gradients not written"
        assert bool((dpos[:, :pred] != 0).any()) == (ws[0] != 0), what
        if skip_dead:
            assert (dpos[:, pred:] == 0).all(), f"{what}: dead steps' dpos not exactly 0"
        elif R > pred:
            assert bool((dpos[:, pred:] != 0).any()) == (ws[1] != 0), f"{what}: extrapolation steps' dpos"


@pytest.mark.parametrize("K,H", SHAPES)
def test_decoder_bwd_lw_mode2_byte_targets(K, H):
    """uint8 targets through the row index (paig_decoder_bwd_t8's form) under
    lw_mode 2: the same bits as the fp32 run on byte / 255 frames."""
    dims = (3, 5, 7, 4)
    c = _case(K, H, *dims, 2)
    adj_dev, adj = _adjoints(("dt", "de"))
    f32 = _bwd_ex(c, 2, adj_dev, 2.0, dims)
    u8 = _bwd_ex(c, 2, adj_dev, 2.0, dims, tgt="tgt8_view")
    assert torch.equal(f32[0], u8[0]) and torch.equal(f32[1], u8[1])
    w = _host_weights(adj, 2.0, *dims)[1]
    _check_ref(c, u8, [w[0], w[dims[3]]], f"byte targets K={K} H={H}")
    assert bool((u8[0] != 0).any())


def test_decoder_bwd_ex_argument_checks():
    """Misuse returns an error code and a message; nothing is launched."""
    lib = L()
    dims = (3, 5, 7, 4)
    adj_dev, _ = _adjoints(("dt",))
    c1, c2 = _case(2, 32, *dims, 1), _case(2, 32, *dims, 2)
    wrec, _ = _loss_bwd(adj_dev, 2.0, *dims)
    # loss adjoints next to a weight array
    assert _bwd_ex(c1, 0, adj_dev, 2.0, dims, dsse=wrec, raw=True) != 0
    assert b"lw_mode 0" in lib.paig_last_error()
    # rollout weights on frames that are not grouped by R
    assert _bwd_ex(c2, 2, adj_dev, 2.0, (3, 5, 21, 4), raw=True) != 0
    assert b"grouped by R" in lib.paig_last_error()
    assert _bwd_ex(c1, 2, adj_dev, 2.0, dims, raw=True) != 0
    assert b"grouped by R" in lib.paig_last_error()
    # in-kernel weights exist for the one-CU shapes only
    K, H = 2, 48
    assert lib.paig_decoder_bwd_blocks(dims[0] * dims[1], 0, 0, K, H // 2, H) >= 1
    tmpl, cont, bg = _sources(K, H, 5)
    F_ = dims[0] * dims[1]
    pos, tgt = _positions(F_, K, H, 3).to(DEV).contiguous(), torch.zeros(F_, 3, H, H, device=DEV)
    c3 = {"K": K, "H": H, "F": F_, "fr": 3 * H * H, "src": [t.to(DEV).contiguous() for t in (tmpl, cont, bg)],
          "pos_view": (pos.data_ptr(), 0, 2 * K, 0), "tgt_view": (tgt.data_ptr(), 3 * H * H, 0, 0)}
    assert _bwd_ex(c3, 1, adj_dev, 2.0, dims, raw=True) != 0
    assert b"one-CU" in lib.paig_last_error()
