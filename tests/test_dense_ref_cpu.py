"""CPU checks of tests/dense_ref.py, the float64 reference the GPU tests of the
dense-tail, velocity-MLP, VFN and mask-softmax kernels compare with: every
hand-written backward against torch autograd of the same forward in float64
(normwise <= 1e-12), and the layouts against the header's index formulas spelt
out element by element.  No GPU."""
import pytest
import torch

import dense_ref as R
from helpers import rel_err

TOL = 1e-12
F64 = torch.float64


def _rnd(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F64) * 2 - 1


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _close(got, want, what):
    assert float(want.abs().max()) > 0, f"{what}: vacuous (zero reference)"
    e = rel_err(got, want.detach())
    assert e <= TOL, f"{what}: {e:.2e}"


@pytest.mark.parametrize("alt", [0, 1])
def test_vel_pack_layout_and_adjoint(alt):
    B, Te, K, S = 3, 5, 3, 3
    g = torch.Generator().manual_seed(1)
    pos = _leaf(_rnd(g, B, Te, 2 * K))
    X = R.vel_pack(pos, K, S, alt)
    cols = 2 * (S - 1 if alt else S)
    assert X.shape == (K * B, cols)
    for k in range(K):
        for b in range(B):
            for t in range(cols // 2):
                for j in range(2):
                    p = pos.detach()
                    want = p[b, t + 1, 2 * k + j] - p[b, t, 2 * k + j] if alt else p[b, t, 2 * k + j]
                    assert float(X.detach()[k * B + b, 2 * t + j]) == float(want)
    dX, dpos0 = _rnd(g, K * B, cols), _rnd(g, B, 2 * K)
    ((X * dX).sum() + (pos[:, S - 1] * dpos0).sum()).backward()
    _close(R.vel_unpack(dX, dpos0, B, Te, K, S, alt), pos.grad, "vel_unpack")
    _close(R.vel_unpack(dX, None, B, Te, K, S, alt) + R.vel_unpack(None, dpos0, B, Te, K, S, alt), pos.grad, "parts")


@pytest.mark.parametrize("B,Te,K,S", [(1, 4, 2, 4), (5, 6, 3, 3), (3, 8, 2, 8), (7, 3, 2, 1)])
def test_velmlp_backward(B, Te, K, S):
    g = torch.Generator().manual_seed(2)
    pos = _rnd(g, B, Te, 2 * K)
    W = [_leaf(_rnd(g, *s)) for s in ((R.HID, 2 * S), (R.HID,), (R.HID, R.HID), (R.HID,), (2, R.HID), (2,))]
    X = _leaf(R.vel_pack(pos, K, S))
    h1 = torch.tanh(X @ W[0].T + W[1])
    h2 = torch.tanh(h1 @ W[2].T + W[3])
    vel = h2 @ W[4].T + W[5]
    Xf, h1f, h2f, velf = R.velmlp_fwd(pos, K, S, *W)
    for a, b in ((Xf, X), (h1f, h1), (h2f, h2), (velf, vel)):
        assert torch.equal(a.detach(), b.detach())
    assert velf.shape == (K * B, 2)
    dvel = _rnd(g, K * B, 2)
    (vel * dvel).sum().backward()
    dX, grads = R.velmlp_bwd(dvel, X.detach(), h1.detach(), h2.detach(), W[0].detach(), W[2].detach(), W[4].detach())
    _close(dX, X.grad, "dX")
    for i, (got, w) in enumerate(zip(grads, W)):
        assert got.shape == w.shape
        _close(got, w.grad, f"velmlp grad {i}")


@pytest.mark.parametrize("P", [1, 9, 288])
@pytest.mark.parametrize("sig", [0, 1])
def test_vfn_backward(P, sig):
    g = torch.Generator().manual_seed(3)
    W1, b1, W2, b2 = (_leaf(_rnd(g, *s) * 0.3) for s in ((R.VH, R.VIN), (R.VH,), (P, R.VH), (P,)))
    h, y, yp = R.vfn_fwd(W1, b1, W2, b2)
    assert h.shape == (R.VH,) and y.shape == (P,)
    assert float((yp - 1 / (1 + torch.exp(-y))).abs().max()) <= 1e-15
    d = _rnd(g, P)
    ((yp if sig else y) * d).sum().backward()
    dW1, db1, dW2, db2, _ = R.vfn_bwd(d, y.detach(), sig, h.detach(), W2.detach())
    for got, w, n in ((dW1, W1, "dW1"), (db1, b1, "db1"), (dW2, W2, "dW2"), (db2, b2, "db2")):
        assert got.shape == w.shape
        _close(got, w.grad, n)


@pytest.mark.parametrize("N,K", [(5, 2), (5, 3)])
def test_pos_head(N, K):
    g = torch.Generator().manual_seed(4)
    h3 = _leaf(_rnd(g, K * N, 2))
    pos = R.pos_head_fwd(h3, N, K, 16.0)
    for f in range(N):
        for k in range(K):
            for j in range(2):
                assert float(pos.detach()[f, 2 * k + j]) == float(torch.tanh(h3.detach()[k * N + f, j]) * 16.0 + 16.0)
    dpos = _rnd(g, N, 2 * K)
    (pos * dpos).sum().backward()
    _close(R.pos_head_bwd(h3.detach(), dpos, N, K, 16.0), h3.grad, "dh3")


def _relu_act(g, *shape):
    """a ReLU's output: exact zeros in about half the entries"""
    return torch.relu(_rnd(g, *shape))


@pytest.mark.parametrize("K,B,Te,S,IN,alt,which", [(2, 3, 5, 3, 20, 0, 3), (3, 3, 5, 3, 24, 1, 3), (2, 3, 5, 3, 8, 1, 1),
                                                  (3, 3, 5, 3, 8, 0, 2), (3, 1, 5, 1, 8, 0, 3), (2, 2, 4, 3, 4, 0, 0)])
def test_head_backward_with_velocity_term(K, B, Te, S, IN, alt, which):
    """which: bit 0 a dX, bit 1 a dpos0; 0: the plain head backward"""
    g = torch.Generator().manual_seed(5)
    F = B * Te
    h2 = _leaf(_relu_act(g, K * F, IN))
    assert 0.3 < float((h2 == 0).double().mean()) < 0.7
    W3, b3 = _leaf(_rnd(g, 2, IN)), _leaf(_rnd(g, 2))
    h3, pos = R.head_fwd(h2, W3, b3, F, K, 16.0)
    cols = 2 * (S - 1 if alt else S)
    dpos = _rnd(g, F, 2 * K)
    dX = _rnd(g, K * B, cols) if which & 1 else None
    dpos0 = _rnd(g, B, 2 * K) if which & 2 else None
    loss = (pos * dpos).sum()
    p3 = pos.reshape(B, Te, 2 * K)
    if dX is not None:
        loss = loss + (R.vel_pack(p3, K, S, alt) * dX).sum()
    if dpos0 is not None:
        loss = loss + (p3[:, S - 1] * dpos0).sum()
    loss.backward()
    vel = (dX, dpos0, B, Te, S, alt) if which else None
    dh2, dW3, db3 = R.head_bwd(h2.detach(), h3.detach(), dpos, W3.detach(), F, K, 16.0, vel)
    # autograd has no ReLU in this graph: l2's ReLU' (h2 > 0) is the mask of the hand-written form
    _close(dh2, h2.grad * (h2.detach() > 0), "dh2")
    assert bool((dh2[h2.detach() == 0] == 0).all())
    _close(dW3, W3.grad, "dW3")
    _close(db3, b3.grad, "db3")


@pytest.mark.parametrize("K,F,IN,S", [(2, 1, 4, 1), (3, 5, 24, 9), (2, 8, 200, 17)])
def test_dense_tail_and_l2_backward(K, F, IN, S):
    g = torch.Generator().manual_seed(6)
    part = _leaf(_rnd(g, S, K * F, IN))
    b1, W2, b2, W3, b3 = (_leaf(_rnd(g, *s) * 0.5) for s in ((IN,), (IN, IN), (IN,), (2, IN), (2,)))
    h1, h2, h3, pos = R.dense_tail_fwd(part, b1, W2, b2, W3, b3, F, K, 16.0)
    assert h1.shape == h2.shape == (K * F, IN) and h3.shape == (K * F, 2) and pos.shape == (F, 2 * K)
    for n in range(K * F):
        want = torch.tanh(h3.detach()[n]) * 16.0 + 16.0
        assert float((pos.detach()[n % F, 2 * (n // F):2 * (n // F) + 2] - want).abs().max()) == 0
    dpos = _rnd(g, F, 2 * K)
    (pos * dpos).sum().backward()
    dh2, dW3, db3 = R.head_bwd(h2.detach(), h3.detach(), dpos, W3.detach(), F, K, 16.0)
    dh1 = R.l2_bwd(dh2, W2.detach(), h1.detach())
    _close(dW3, W3.grad, "dW3")
    _close(db3, b3.grad, "db3")
    _close(dh2.T @ h1.detach(), W2.grad, "dW2 from dh2")
    _close(dh2.sum(0), b2.grad, "db2 from dh2")
    _close(dh1.sum(0), b1.grad, "db1 from dh1")
    for s in range(S):
        _close(dh1, part.grad[s], "dh1")


@pytest.mark.parametrize("F,K,C,H,W", [(1, 2, 3, 4, 4), (5, 3, 3, 4, 6), (1, 1, 1, 4, 4), (5, 7, 3, 2, 2)])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_mask_softmax_backward(F, K, C, H, W, flags):
    g = torch.Generator().manual_seed(7)
    pre = _leaf(_rnd(g, F, K, H, W) * 3)
    logits = torch.relu(pre) if flags & 1 else pre
    x = _rnd(g, F, C, H, W)
    masks, objs, pobjs = R.mask_softmax_fwd(logits, x, pool=bool(flags & 2))
    assert masks.shape == (F, K + 1, H, W) and objs.shape == (K * F, C, H, W)
    assert float((masks.sum(1) - 1).abs().max()) <= 1e-14
    for k in range(K):
        assert torch.equal(objs[k * F:(k + 1) * F].detach(), (masks[:, k:k + 1] * x).detach())
    out = pobjs if flags & 2 else objs
    if flags & 2:
        assert float((pobjs - torch.nn.functional.avg_pool2d(objs, 2)).abs().max()) <= 1e-15
    d = _rnd(g, *out.shape)
    (out * d).sum().backward()
    got = R.mask_softmax_bwd(logits.detach(), x, masks.detach(), d, flags)
    _close(got, pre.grad, "dlogits")
    if flags & 1:
        assert bool((got[logits.detach() == 0] == 0).all()) and bool((logits == 0).any())


def test_colsum():
    g = torch.Generator().manual_seed(8)
    X, o = _rnd(g, 7, 5), _rnd(g, 5)
    assert float((R.colsum(X) - X.T @ torch.ones(7, dtype=F64)).abs().max()) <= 1e-14
    assert torch.equal(R.colsum(X, o), R.colsum(X) + o)
