"""synth_device's host half (no GPU): integrate_host is pinned to synth.py's
integrators, initial_conditions draws the right shapes and ranges, the C ABI
refuses object counts it has no kernel for, and the seeds the GPU tests use
leave no acceptance flag to rounding."""
import numpy as np
import pytest

from paig_reproduction_amd import _lib
from paig_reproduction_amd.nn.datasets import synth
from paig_reproduction_amd.nn.datasets import synth_device as SD

import synth_device_ref as R

# seeds whose first draw synth._spring_traj accepts (T = 12, size 32)
SPRING_SEEDS = (2, 3, 4, 6, 11, 15, 17, 18)


def _spring_draw(rng, size, radius, equil=6.0, vmax=8.0):
    """The first draw of synth._spring_traj (:41-50), in its RNG order."""
    lo, hi = radius + equil, size - (radius + equil)
    cm = lo + (hi - lo) * rng.random(2)
    ang = rng.random() * 2 * np.pi
    r = rng.random() + 0.5
    p = np.array([[np.cos(ang) * equil * r, np.sin(ang) * equil * r],
                  [-np.cos(ang) * equil * r, -np.sin(ang) * equil * r]]) + cm
    a = rng.random(2) * 2 * np.pi
    v = np.stack([np.cos(a) * vmax, np.sin(a) * vmax], axis=1) * rng.random((2, 1))
    return p, v


def _bounce_draw(rng, size, radius, vmax=8.0):
    p = radius + (size - 2 * radius) * rng.random((2, 2))
    a = rng.random(2) * 2 * np.pi
    v = np.stack([np.cos(a), np.sin(a)], axis=1) * vmax * (0.5 + 0.5 * rng.random((2, 1)))
    return p, v


def _gravity_draw(rng, size, g=60.0):
    c = size / 2
    ang = rng.random() * 2 * np.pi + np.array([0, 2 * np.pi / 3, 4 * np.pi / 3])
    r = 4 + 4 * rng.random()
    p = np.stack([c + r * np.cos(ang), c + r * np.sin(ang)], axis=1)
    v = np.stack([-np.sin(ang), np.cos(ang)], axis=1) * (np.sqrt(g / r) * 0.35)
    return p, v


@pytest.mark.parametrize("seed", SPRING_SEEDS)
def test_integrate_host_matches_spring_traj(seed):
    want = synth._spring_traj(np.random.default_rng(seed), 12, 32, 2.0)
    p, v = _spring_draw(np.random.default_rng(seed), 32, 2.0)
    pos, valid = SD.integrate_host("spring_color", p[None], v[None], 12)
    assert valid[0]                                   # the first draw is the one the host kept
    assert pos.shape == (1, 12, 2, 2) and pos.dtype == np.float64
    assert np.abs(pos[0] - want).max() <= 1e-10


@pytest.mark.parametrize("seed", range(8))
def test_integrate_host_matches_bounce_traj(seed):
    want = synth._bounce_traj(np.random.default_rng(seed), 100, 32, 2.0)
    p, v = _bounce_draw(np.random.default_rng(seed), 32, 2.0)
    pos, valid = SD.integrate_host("bouncing_balls", p[None], v[None], 100)
    assert valid[0]
    assert np.abs(pos[0] - want).max() <= 1e-10


@pytest.mark.parametrize("seed", range(8))
def test_integrate_host_matches_gravity_traj(seed):
    """Three bodies are chaotic: the bound is the envelope of the GPU test,
    16 x the trajectory's own float64-vs-longdouble spread (floor 1e-12 px)."""
    T = 40
    want = synth._gravity_traj(np.random.default_rng(seed), T, 36, 2.0)
    p, v = _gravity_draw(np.random.default_rng(seed), 36)
    pos, valid, tol, _ = R.host_envelope("3bp_color", p[None], v[None], T)
    assert valid[0]
    err = np.abs(pos[0] - want).max()
    print(f"gravity seed {seed}: |integrate_host - _gravity_traj| = {err:.3e}, bound {tol[0]:.3e}")
    assert err <= tol[0]


def test_longdouble_is_accepted_and_close():
    p0, v0 = SD.initial_conditions("spring_color", np.random.default_rng(0), 8)
    p64, ok64 = SD.integrate_host("spring_color", p0, v0, 12)
    pld, okld = SD.integrate_host("spring_color", p0, v0, 12, dtype=np.longdouble)
    assert pld.dtype == np.longdouble and np.array_equal(ok64, okld)
    assert np.abs(p64 - pld).max() < 1e-9


@pytest.mark.parametrize("task", sorted(synth.TASKS))
def test_initial_conditions_shapes_and_ranges(task):
    K, size, phys = synth.TASKS[task]
    q = SD.task_params(task)
    m = 257
    p0, v0 = SD.initial_conditions(task, np.random.default_rng(1), m)
    assert p0.shape == (m, K, 2) and v0.shape == (m, K, 2)
    assert p0.dtype == np.float64 and v0.dtype == np.float64
    assert p0.flags.c_contiguous and v0.flags.c_contiguous
    rb = q["bound"]
    if phys == "gravity":
        # radius 4..8 around the centre: strictly inside the frame bounds
        assert (p0 > rb).all() and (p0 < size - rb).all()
        r = np.linalg.norm(p0 - size / 2, axis=2)
        assert (r >= 4 - 1e-9).all() and (r < 8 + 1e-9).all()
    elif phys == "bounce":
        assert (p0 >= rb).all() and (p0 <= size - rb).all()
        sp = np.linalg.norm(v0, axis=2)
        assert (sp >= 4 - 1e-9).all() and (sp <= 8 + 1e-9).all()
    else:
        # the centre of mass lies inside the frame bounds with the spring's rest
        # length to spare, the objects half a separation (0.5..1.5 equil) from it.
        # As in synth._spring_traj a start can therefore reach up to equil / 2
        # past a bound; the acceptance rule deals with those.
        equil = q["c1"]
        cm = p0.mean(axis=1)
        assert (cm >= rb + equil - 1e-9).all() and (cm <= size - rb - equil + 1e-9).all()
        if q["half"]:
            assert (cm[:, 0] <= size / 2 + 1e-9).all()
        sep = np.linalg.norm(p0[:, 0] - p0[:, 1], axis=1)
        assert (sep >= equil - 1e-9).all() and (sep <= 3 * equil + 1e-9).all()
        assert (p0 >= rb - equil / 2 - 1e-9).all() and (p0 <= size - rb + equil / 2 + 1e-9).all()
        assert (np.linalg.norm(v0, axis=2) <= 8 + 1e-9).all()
    # mnist: frame bounds at radius * 2, disks drawn at radius * 3, rest length 12
    if task == "mnist_spring_color":
        assert (q["bound"], q["draw"], q["c1"]) == (4.0, 6.0, 12.0)


def test_initial_conditions_is_a_stream():
    """Rounds of a fixed size from one generator: what the prefix property of
    render_sequences_device rests on."""
    a = SD.initial_conditions("spring_color", np.random.default_rng(5), 16)
    b = SD.initial_conditions("spring_color", np.random.default_rng(5), 16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("task,T,seed", [("spring_color", 12, 0), ("bouncing_balls", 30, 0), ("3bp_color", 20, 0)])
def test_gpu_integrator_seed_skips_no_candidate(task, T, seed):
    """The GPU integrator test may skip a candidate whose acceptance hangs on
    rounding (host margin < tolerance); for its seed none does."""
    p0, v0 = SD.initial_conditions(task, np.random.default_rng(seed), 64)
    _, valid, tol, margin = R.host_envelope(task, p0, v0, T)
    assert (margin >= tol).all(), (margin.min(), tol.max())
    print(f"{task}: {int(valid.sum())} of 64 accepted, max tol {tol.max():.3e}, min margin {margin.min():.3e}")


@pytest.mark.parametrize("n,T,chunk", [(6, 12, 4096), (3, 50, 16)])
def test_gpu_end_to_end_seed_is_unambiguous(n, T, chunk):
    pos, tol, slack, drawn = R.host_select("spring_color", n, T, 3, chunk)
    assert len(pos) == n and slack > 0
    if chunk == 16:
        assert drawn > chunk                # several rounds, as the GPU test wants
    print(f"T={T}: {n} accepted of {drawn} drawn")


def test_abi_refuses_unsupported_object_counts():
    """K outside {2, 3}, or not the physics' own count, is an error return
    before any launch (no GPU needed)."""
    L = _lib.lib()
    for phys, K in ((0, 3), (1, 3), (2, 2), (0, 4), (1, 1), (3, 2)):
        with pytest.raises(_lib.PaigError):
            L.paig_synth_integrate(phys, None, None, 4, K, 3, 10, 0.3, 32.0, 2.0, 4.0, 6.0, None, None, None)
    for K, size in ((1, 32), (4, 32), (2, 30)):
        with pytest.raises(_lib.PaigError):
            L.paig_synth_raster(None, None, 2, 3, K, size, 2.0, None, None, None)


def test_device_wrappers_refuse_cpu_tensors():
    import torch
    z = torch.zeros((4, 2, 2), dtype=torch.float64)
    with pytest.raises(_lib.PaigError):
        SD.integrate_device("spring_color", z, z, 3)
    with pytest.raises(_lib.PaigError):
        SD.rasterize_device(torch.zeros((4, 3, 2, 2), dtype=torch.float64), 32, 2.0)
