"""Which conv kernel answers for a shape, characterised from the host: the three
queries csrc/unet.hip plans the network from (paig_conv2d_mfma_supported,
paig_conv2d_bwd_supported; paig_conv_split_supported answers through the
first) over a grid of shapes and flags, and the plans that consume them.  The
answers were recorded from the library before the kernel routing became one
resolver per kernel family (tests/golden/conv_routing.json) and must not move:
a plan laid out from one answer and launched by another gets buffers it was
never sized for.  Pure host functions: no GPU."""
import pytest

import conv_routing_grid as G
from paig_reproduction_amd import _lib


def _diff(got, want):
    got, want = {tuple(p) for p in got}, {tuple(p) for p in want}
    for p in sorted(got - want):
        print("accepted now, refused when recorded:", p)
    for p in sorted(want - got):
        print("refused now, accepted when recorded:", p)
    return got == want


def test_mfma_supported_accepts_the_recorded_points():
    assert _diff(G.mfma_accepted(_lib.lib()), G.golden()["mfma_supported"])


def test_bwd_supported_accepts_the_recorded_points():
    assert _diff(G.bwd_accepted(_lib.lib()), G.golden()["bwd_supported"])


def test_unet_plans_match_the_recorded_layouts():
    got, want = G.unet_plans(_lib.lib()), G.golden()["unet_plans"]
    assert set(got) == set(want)
    moved = [k for k in want if got[k] != want[k]]
    for k in moved:
        print("net H K cm flags =", k, "\n  recorded", want[k], "\n  now     ", got[k])
    assert not moved
