"""paig_grad_norm through the C ABI on synthetic buffers: per-segment squared
sums, total norm, clip coefficient and the sticky non-finite flag against
float64 on the CPU.

Bars (derived, not measured): the square of an fp32 value is exact in fp64, so
sq[i] carries only the rounding of at most len_i fp64 additions, each at most
2^-53 relative to a partial sum that never exceeds the (all-positive) total:
|sq[i] - exact| <= len_i * 2^-53 * sq[i].  The float64 reference sum has the
same bound, so the two may differ by len_i * 2^-52 relative.  The same holds
for the total over n elements; sqrt halves a relative error and the division
of the coefficient adds roundings far below n * 2^-52's slack only for n >= 2,
and for n = 1 every operation (one exact product, IEEE sqrt, add, divide) is
the same correctly rounded operation on both sides.
"""
import math

import pytest
import torch

from paig_reproduction_amd import _lib
from paig_reproduction_amd._lib import GN_COEF, GN_GROUP0, GN_NONFINITE, GN_NORM, GN_SQ0, GN_TOTAL_SQ, lib, ptr
from paig_reproduction_amd.flat import segment_table

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS = 2.0 ** -52


class Norm:
    """Device buffers of one problem: launch() fills and returns stats."""

    def __init__(self, g32, g64, segs, groups=None):
        L = lib()
        self.g32 = g32.to(DEV)
        self.g64 = g64.to(DEV) if g64 is not None and g64.numel() else None
        self.n32, self.n64 = g32.numel(), 0 if g64 is None else g64.numel()
        groups = groups or [-1] * len(segs)
        table, self.nchunks = segment_table([(k, o, n, g) for (k, o, n), g in zip(segs, groups)],
                                            L.paig_grad_norm_chunk())
        self.table = table.to(DEV)
        self.nseg = len(segs)
        self.stats = torch.zeros(GN_SQ0 + self.nseg, device=DEV, dtype=torch.float64)
        self.scratch = torch.empty(L.paig_grad_norm_scratch(self.nchunks) // 8, device=DEV, dtype=torch.float64)

    def launch(self, max_norm=0.0, mask=None):
        self.mask = None if mask is None else torch.tensor(mask, dtype=torch.uint8, device=DEV)
        lib().paig_grad_norm(ptr(self.g32), self.n32, ptr(self.g64), self.n64, ptr(self.table), self.nseg,
                             self.nchunks, ptr(self.mask), float(max_norm), ptr(self.stats), ptr(self.scratch),
                             self.scratch.numel() * 8, _lib.stream_handle(DEV))
        return self.stats

    def read(self, max_norm=0.0, mask=None):
        s = self.launch(max_norm, mask)
        torch.cuda.synchronize()
        return s.cpu().clone()


def reference(g32, g64, segs, max_norm, mask=None):
    """float64 on the CPU: per-segment (g.double() ** 2).sum(), the total in
    index order, torch's clip_grad_norm_ coefficient."""
    sq = []
    for i, (kind, off, num) in enumerate(segs):
        g = (g32 if kind == 32 else g64)[off:off + num]
        sq.append(float((g.double() ** 2).sum()) if mask is None or mask[i] else 0.0)
    tot = 0.0
    for v in sq:
        tot += v
    norm = math.sqrt(tot) if tot == tot and tot >= 0 else float("nan")
    coef = 1.0
    if max_norm > 0:
        coef = float(torch.clamp(torch.tensor(max_norm / (norm + 1e-6), dtype=torch.float64), max=1.0))
    return sq, norm, coef


def _single(n32, n64):
    segs = [(32, 0, n32)] + [(64, i, 1) for i in range(n64)]
    return n32, n64, segs


def _tiny300():
    gen = torch.Generator().manual_seed(5)
    lens = torch.randint(1, 6, (300,), generator=gen).tolist()
    gaps = torch.randint(0, 3, (300,), generator=gen).tolist()
    segs, off = [], 1
    for n, gap in zip(lens, gaps):
        segs.append((32, off, n))
        off += n + gap
    return off + 3, 1, segs + [(64, 0, 1)]


CASES = {
    **{f"n32_{n}_n64_{k}": _single(n, k) for n, k in zip((1, 63, 64, 65, 255, 256, 257), (0, 1, 2, 0, 1, 2, 0))},
    # one segment over 18 blocks (17 full chunks + 369 elements), misaligned by 3 elements
    "one_segment_70001": (70010, 2, [(32, 3, 70001), (64, 0, 2)]),
    "tiny_300_odd_offsets": _tiny300(),
    # the table starts at element 1: every 16-byte interior starts after a 3-element head
    "first_segment_at_1": (9000, 0, [(32, 1, 4099), (32, 4100, 2), (32, 4102, 4898)]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_shapes_against_float64(case):
    n32, n64, segs = CASES[case]
    gen = torch.Generator().manual_seed(len(case))
    g32 = torch.randn(n32, generator=gen) * torch.logspace(-3, 3, n32)[torch.randperm(n32, generator=gen)]
    g64 = torch.randn(max(n64, 1), generator=gen, dtype=torch.float64)[:n64]
    groups = [i % 3 for i in range(len(segs))]
    P = Norm(g32, g64, segs, groups)
    n = sum(s[2] for s in segs)
    rsq, rnorm, _ = reference(g32, g64, segs, 0.0)
    for max_norm in (0.0, 0.5 * rnorm, 2.0 * rnorm):
        _, _, rcoef = reference(g32, g64, segs, max_norm)
        st = P.read(max_norm)
        for i, (_, _, num) in enumerate(segs):
            got = float(st[GN_SQ0 + i])
            print(case, "sq", i, got, rsq[i])
            assert abs(got - rsq[i]) <= num * EPS * rsq[i], (case, i, got, rsq[i])
        print(case, "norm", float(st[GN_NORM]), rnorm, "coef", float(st[GN_COEF]), rcoef)
        assert abs(float(st[GN_NORM]) - rnorm) <= n * EPS * rnorm, (case, float(st[GN_NORM]), rnorm)
        assert abs(float(st[GN_COEF]) - rcoef) <= n * EPS * rcoef, (case, float(st[GN_COEF]), rcoef)
        if max_norm == 0.0 or max_norm > rnorm:
            assert float(st[GN_COEF]) == 1.0
        assert float(st[GN_NONFINITE]) == 0.0
        assert abs(float(st[GN_TOTAL_SQ]) - rnorm ** 2) <= 2 * n * EPS * rnorm ** 2
        # the in-kernel group sums: the same segments' sq, by group
        for g in range(3):
            want = math.sqrt(sum(rsq[i] for i in range(len(segs)) if groups[i] == g))
            cnt = sum(segs[i][2] for i in range(len(segs)) if groups[i] == g)
            assert abs(float(st[GN_GROUP0 + g]) - want) <= max(cnt, 1) * EPS * want


def test_range_beyond_fp32():
    """|g| in [1e18, 3e19] over 100k elements: the sum of squares (~1e43) is
    far beyond fp32's range, the fp64 norm is finite and on the bar."""
    n = 100_000
    gen = torch.Generator().manual_seed(1)
    g32 = (1e18 + torch.rand(n, generator=gen, dtype=torch.float64) * 2.9e19).float()
    g32 *= torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    segs = [(32, 0, 60_001), (32, 60_001, n - 60_001)]
    rsq, rnorm, rcoef = reference(g32, None, segs, 1.0)
    assert rnorm ** 2 > 3.5e38 and math.isfinite(rnorm)
    st = Norm(g32, None, segs).read(1.0)
    assert abs(float(st[GN_NORM]) - rnorm) <= n * EPS * rnorm
    assert abs(float(st[GN_COEF]) - rcoef) <= n * EPS * rcoef
    assert float(st[GN_NONFINITE]) == 0.0


def test_all_zero_gradients():
    st = Norm(torch.zeros(1000), torch.zeros(2, dtype=torch.float64), [(32, 0, 999), (64, 0, 2)]).read(1.0)
    assert float(st[GN_NORM]) == 0.0 and float(st[GN_COEF]) == 1.0 and float(st[GN_NONFINITE]) == 0.0


def test_masked_segments_are_never_read():
    gen = torch.Generator().manual_seed(2)
    g32 = torch.randn(10_000, generator=gen)
    g64 = torch.randn(2, generator=gen, dtype=torch.float64)
    segs = [(32, 0, 5000), (32, 5000, 4500), (32, 9500, 500), (64, 0, 1), (64, 1, 1)]
    mask = [1, 0, 1, 0, 1]
    clean = Norm(g32, g64, segs).read(0.3, mask)
    bad32, bad64 = g32.clone(), g64.clone()
    bad32[5000:9500] = float("nan")
    bad64[0] = float("nan")
    got = Norm(bad32, bad64, segs).read(0.3, mask)
    assert torch.equal(got.view(torch.int64), clean.view(torch.int64))
    assert float(got[GN_SQ0 + 1]) == 0.0 and float(got[GN_SQ0 + 3]) == 0.0 and float(got[GN_NONFINITE]) == 0.0
    rsq, rnorm, rcoef = reference(g32, g64, segs, 0.3, mask)
    assert abs(float(got[GN_NORM]) - rnorm) <= 5501 * EPS * rnorm


def test_nonfinite_flag_is_sticky():
    gen = torch.Generator().manual_seed(3)
    g32 = torch.randn(3000, generator=gen)
    segs = [(32, 0, 1000), (32, 1000, 2000)]
    P = Norm(g32, None, segs)
    P.g32[1234] = float("inf")
    st = P.read(1.0)
    assert not math.isfinite(float(st[GN_NORM])) and float(st[GN_NONFINITE]) == 1.0
    assert float(st[GN_COEF]) == 0.0          # torch: 1 / (inf + 1e-6) = 0
    P.g32[1234] = float("nan")
    st = P.read(1.0)
    assert math.isnan(float(st[GN_NORM])) and math.isnan(float(st[GN_COEF]))   # error_if_nonfinite=False: NaN propagates
    P.g32[1234] = 0.5
    st = P.read(1.0)                           # a clean launch leaves the flag set
    assert math.isfinite(float(st[GN_NORM])) and float(st[GN_NONFINITE]) == 1.0
    P.stats[GN_NONFINITE].zero_()              # the host clears it
    st = P.read(1.0)
    assert float(st[GN_NONFINITE]) == 0.0


def test_deterministic_eager_and_graph_replay():
    n32, n64, segs = CASES["one_segment_70001"]
    gen = torch.Generator().manual_seed(4)
    g32 = torch.randn(n32, generator=gen)
    g64 = torch.randn(n64, generator=gen, dtype=torch.float64)
    P = Norm(g32, g64, segs + [(32, 0, 3)])
    first = P.read(0.7)
    for _ in range(9):
        P.stats.zero_()
        assert torch.equal(P.read(0.7).view(torch.int64), first.view(torch.int64))
    P.stats.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        P.launch(0.7)
    torch.cuda.synchronize()
    P.stats.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(P.stats.cpu().view(torch.int64), first.view(torch.int64))
