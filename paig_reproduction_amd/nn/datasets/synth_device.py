"""Synthetic datasets rendered on the device (csrc/synth.hip).

``synth.py`` renders one sequence at a time in a Python loop and redraws a
trajectory until it stays in frame.  Here the candidates of a whole round are
drawn at once on the host (vectorised numpy), integrated on the GPU one lane
each (``paig_synth_integrate``, fp64, the host's update order and acceptance
rule) and the accepted ones rasterised straight into the uint8 NHWC dataset
tensor (``paig_synth_raster``, bit for bit ``synth._disk_frames`` and the
composition of ``synth.render_sequences``).  The result stays in HBM, where
``DeviceDataIterator`` reads it.

The device renderer does NOT replay ``synth.py``'s RNG stream: it produces
*different* sequences from ``render_sequences(seed)``, drawn from the same
distribution.  ``synth.py`` and everything rendered through it are unchanged.

``integrate_host`` is the same integrators in plain numpy for explicit
initial states: the test reference, no GPU needed.
"""
import numpy as np

from .synth import TASKS

PHYS_ID = {"spring": 0, "bounce": 1, "gravity": 2}


def task_params(task, radius=2.0):
    """The per-task constants of ``render_sequences`` (synth.py:115-125) and of
    the integrators' defaults: ``bound`` is the radius of the frame bounds,
    ``draw`` the radius of the drawn disks."""
    K, size, phys = TASKS[task]
    if phys == "spring":
        scale = size / 32.0
        return dict(phys=phys, K=K, size=size, bound=radius * scale, draw=radius * (3.0 if task == "mnist_spring_color" else 1.0),
                    c0=4.0, c1=6.0 * scale, dt=0.3, sub=10, vmax=8.0, half=(task == "spring_color_half"))
    if phys == "bounce":
        return dict(phys=phys, K=K, size=size, bound=radius, draw=radius, c0=0.0, c1=0.0, dt=0.3, sub=10, vmax=8.0)
    return dict(phys=phys, K=K, size=size, bound=radius, draw=radius, c0=60.0, c1=0.0, dt=0.5, sub=10)


def initial_conditions(task, rng, m, radius=2.0):
    """``m`` candidate initial states -> (p0, v0), float64 [m, K, 2].

    Vectorised draws from the distributions of ``_spring_traj`` (synth.py:41-50,
    ``half`` included), ``_bounce_traj`` (:70-72) and ``_gravity_traj`` (:87-91)
    with the per-task scaling of ``render_sequences``.  The draws are NOT the
    RNG stream of ``synth.py``: sequences rendered from them differ from
    ``render_sequences(seed)``; they follow the same distribution."""
    q = task_params(task, radius)
    size, rb = q["size"], q["bound"]
    if q["phys"] == "spring":
        equil, vmax = q["c1"], q["vmax"]
        lo, hi = rb + equil, size - (rb + equil)
        cm = lo + (hi - lo) * rng.random((m, 2))
        if q["half"]:
            cm[:, 0] = lo + (size / 2 - lo) * rng.random(m)
        ang = rng.random(m) * 2 * np.pi
        r = rng.random(m) + 0.5
        off = np.stack([np.cos(ang) * equil * r, np.sin(ang) * equil * r], axis=1)   # [m, 2]
        p = np.stack([off, -off], axis=1) + cm[:, None, :]
        a = rng.random((m, 2)) * 2 * np.pi
        v = np.stack([np.cos(a) * vmax, np.sin(a) * vmax], axis=2) * rng.random((m, 2, 1))
    elif q["phys"] == "bounce":
        vmax = q["vmax"]
        p = rb + (size - 2 * rb) * rng.random((m, 2, 2))
        a = rng.random((m, 2)) * 2 * np.pi
        v = np.stack([np.cos(a), np.sin(a)], axis=2) * vmax * (0.5 + 0.5 * rng.random((m, 2, 1)))
    else:
        g, c = q["c0"], size / 2
        ang = rng.random(m)[:, None] * 2 * np.pi + np.array([0, 2 * np.pi / 3, 4 * np.pi / 3])   # [m, 3]
        r = (4 + 4 * rng.random(m))[:, None]
        p = np.stack([c + r * np.cos(ang), c + r * np.sin(ang)], axis=2)
        sp = np.sqrt(g / r) * 0.35
        v = np.stack([-np.sin(ang), np.cos(ang)], axis=2) * sp[:, :, None]
    return np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)


# ---- the counter-based draws of paig_synth_draw (csrc/synth.hip) on the host ----
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
DRAW_U = 8          # uniforms per candidate (4 draw slots of 2)
BG_SLOT = 0x6267    # the draw slot of the mnist_spring_color background


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11, the Random123 constants) over
    arrays: ``counter`` [..., 4] and ``key`` [..., 2] (broadcast against each
    other) of 32-bit words -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xffffffff)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(0xffffffff)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j], shape).copy() for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j], shape).copy() for j in range(2))
    mask, s32 = np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        a, b = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2   # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (b >> s32) ^ c1 ^ k0, b & mask, (a >> s32) ^ c3 ^ k1, a & mask
        k0 = (k0 + np.uint64(PHILOX_W0)) & mask
        k1 = (k1 + np.uint64(PHILOX_W1)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def u53(a, b):
    """numpy's double from two 32-bit words: ((a >> 5) 2^26 + (b >> 6)) 2^-53,
    every step exact in float64."""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    return ((a >> np.uint32(5)).astype(np.float64) * 67108864.0 + (b >> np.uint32(6)).astype(np.float64)) * \
        (1.0 / 9007199254740992.0)


def _check_key(seed, stream, round):
    for name, v in (("seed", seed), ("stream", stream), ("round", round)):
        if not 0 <= int(v) < 2 ** 32:
            raise ValueError(f"{name}={v}: must be in [0, 2^32)")


def philox_uniforms(seed, stream, round, m, slots=DRAW_U // 2):
    """float64 [m, 2 * slots]: u[i, 2 s] / u[i, 2 s + 1] from words (0, 1) /
    (2, 3) of the Philox block with key (seed, stream) and counter
    (i low word, i high word, round, s)."""
    _check_key(seed, stream, round)
    i = np.arange(int(m), dtype=np.uint64)[:, None]
    s = np.arange(int(slots), dtype=np.uint64)[None, :]
    ctr = np.stack(np.broadcast_arrays(i & np.uint64(0xffffffff), i >> np.uint64(32), np.uint64(int(round)), s), axis=-1)
    w = philox4x32_10(ctr, np.array([int(seed), int(stream)], dtype=np.uint64))   # [m, slots, 4]
    return np.stack([u53(w[..., 0], w[..., 1]), u53(w[..., 2], w[..., 3])], axis=-1).reshape(int(m), 2 * int(slots))


def initial_conditions_philox(task, seed, stream, round, m, radius=2.0, return_uniforms=False):
    """The host twin of ``paig_synth_draw``: ``m`` candidate initial states
    (p0, v0), float64 [m, K, 2], from the distributions of
    ``initial_conditions``, a pure function of (seed, stream, round, candidate
    index): the first ``a`` candidates of an ``m = b > a`` call are those of
    the ``m = a`` call.  The arithmetic is the kernel's, operation for
    operation; only sin / cos / sqrt come from another library.

    Use of the uniforms u0 .. u7 of a candidate (``philox_uniforms``):
      spring   u0 u1 centre of mass (``half``: x from the left half, same u0);
               u2 pair angle; u3 + 0.5 pair distance / equil; u4 u5 velocity
               angles of objects 0, 1; u6 u7 their speeds / vmax
      bounce   u0 u1 / u2 u3 positions of objects 0 / 1; u4 u5 velocity
               angles; 0.5 + 0.5 u6, 0.5 + 0.5 u7 speeds / vmax
      gravity  u0 angle of object 0; 4 + 4 u1 orbit radius (slot 0 only)"""
    q = task_params(task, radius)
    size, rb = float(q["size"]), float(q["bound"])
    m = int(m)
    u = philox_uniforms(seed, stream, round, m, 1 if q["phys"] == "gravity" else DRAW_U // 2)
    if q["phys"] == "spring":
        equil, vmax = q["c1"], q["vmax"]
        lo, hi = rb + equil, size - (rb + equil)
        cx = lo + (size / 2.0 - lo) * u[:, 0] if q["half"] else lo + (hi - lo) * u[:, 0]
        cy = lo + (hi - lo) * u[:, 1]
        ang, r = u[:, 2] * 2.0 * np.pi, u[:, 3] + 0.5
        ox, oy = np.cos(ang) * equil * r, np.sin(ang) * equil * r
        p = np.stack([np.stack([ox + cx, oy + cy], 1), np.stack([-ox + cx, -oy + cy], 1)], 1)
        a = u[:, 4:6] * 2.0 * np.pi
        v = np.stack([np.cos(a) * vmax * u[:, 6:8], np.sin(a) * vmax * u[:, 6:8]], 2)
    elif q["phys"] == "bounce":
        vmax = q["vmax"]
        p = (rb + (size - 2.0 * rb) * u[:, 0:4]).reshape(m, 2, 2)
        a, s = u[:, 4:6] * 2.0 * np.pi, 0.5 + 0.5 * u[:, 6:8]
        v = np.stack([np.cos(a) * vmax * s, np.sin(a) * vmax * s], 2)
    else:
        c = size / 2.0
        a = (u[:, 0] * 2.0 * np.pi)[:, None] + np.array([0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0])
        r = (4.0 + 4.0 * u[:, 1])[:, None]
        sp = np.sqrt(q["c0"] / r) * 0.35
        cs, sn = np.cos(a), np.sin(a)
        p = np.stack([c + r * cs, c + r * sn], 2)
        v = np.stack([-sn * sp, cs * sp], 2)
        u = np.concatenate([u, np.zeros((m, DRAW_U - 2))], 1)
    p, v = np.ascontiguousarray(p, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    return (p, v, u) if return_uniforms else (p, v)


def background_philox(seed, stream, round, n, size):
    """The host twin of ``paig_synth_background``: float32 [n, size, size]."""
    _check_key(seed, stream, round)
    qn = int(n) * size * size // 4
    qi = np.arange(qn, dtype=np.uint64)
    ctr = np.stack(np.broadcast_arrays(qi & np.uint64(0xffffffff), qi >> np.uint64(32), np.uint64(int(round)),
                                       np.uint64(BG_SLOT)), axis=-1)
    w = philox4x32_10(ctr, np.array([int(seed), int(stream)], dtype=np.uint64))
    uf = (w >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.clip(uf - np.float32(0.2), np.float32(0.0), np.float32(1.0)).reshape(int(n), size, size)


_RATE_CACHE = {}


def acceptance_rate(task, seq_len, m=2048, radius=2.0):
    """The fraction of ``m`` Philox candidates (a fixed key of its own) that
    ``integrate_host`` accepts for sequences of ``seq_len``: measured on the
    CPU, once per (task, seq_len); the same on every rank."""
    key = (task, int(seq_len), int(m), float(radius))
    if key not in _RATE_CACHE:
        p0, v0 = initial_conditions_philox(task, 0x5eed, 0xffffffff, 0, m, radius)
        _RATE_CACHE[key] = float(integrate_host(task, p0, v0, int(seq_len), radius)[1].mean())
    return _RATE_CACHE[key]


def default_candidates(task, seq_len, batch, margin=1.5, radius=2.0):
    """Candidates per refill so that the expected accepted count is at least
    ``margin * batch``, rounded up to whole waves of 64."""
    m = 2048
    rate = max(acceptance_rate(task, seq_len, m, radius), 1.0 / m)
    return int(-(-int(np.ceil(margin * batch / rate)) // 64) * 64)


def integrate_host(task, p0, v0, T, radius=2.0, dtype=np.float64):
    """The integrators of synth.py for explicit initial states, vectorised
    over the candidates: (pos [m, T, K, 2] of ``dtype``, valid bool [m]).

    ``pos[:, t]`` is the state before step t's substeps; ``valid`` is the
    host's acceptance rule (synth.py:62 / :105; bounce accepts everything).
    A rejected candidate is integrated to the end all the same (the host
    stops at the first violation), so its later positions are not the host's.
    ``dtype=np.longdouble`` gives the wider evaluation the tests use to size
    their tolerance."""
    q = task_params(task, radius)
    dt_ = np.dtype(dtype).type
    p = np.array(p0, dtype=dtype)
    v = np.array(v0, dtype=dtype)
    m, K = p.shape[0], q["K"]
    assert p.shape == (m, K, 2) and v.shape == (m, K, 2), (p.shape, v.shape, K)
    h = dt_(q["dt"] / q["sub"])
    lo, hi = dt_(q["bound"]), dt_(q["size"] - q["bound"])
    c0, eq2 = dt_(q["c0"]), dt_(2 * q["c1"])
    pos = np.zeros((m, T, K, 2), dtype=dtype)
    valid = np.ones(m, dtype=bool)
    for t in range(T):
        pos[:, t] = p
        for _ in range(q["sub"]):
            if q["phys"] == "spring":
                d = p[:, 0] - p[:, 1]
                n = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + dt_(1e-8)
                F = (c0 * (n - eq2))[:, None] * d / n[:, None]
                v[:, 0] = v[:, 0] - h * F
                v[:, 1] = v[:, 1] + h * F
                p = p + h * v
            elif q["phys"] == "bounce":
                p = p + h * v
                l, g = p < lo, p > hi
                v = np.where(l | g, -v, v)
                p = np.where(l, 2 * lo - p, np.where(g, 2 * hi - p, p))
            else:
                acc = np.zeros_like(p)
                for i in range(3):
                    for j in range(3):
                        if i != j:
                            d = p[:, j] - p[:, i]
                            n = np.maximum(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]), dt_(1.0))
                            acc[:, i] += c0 * d / (n * n * n)[:, None]
                v = v + h * acc
                p = p + h * v
        if q["phys"] == "spring":
            valid &= ~(np.any(p < lo, axis=(1, 2)) | np.any(p > hi, axis=(1, 2)))
    if q["phys"] == "gravity":
        valid = np.all(pos > lo, axis=(1, 2, 3)) & np.all(pos < hi, axis=(1, 2, 3))
    return pos, valid


def integrate_device(task, p0, v0, T, radius=2.0, pos=None, valid=None):
    """``paig_synth_integrate`` on the current stream: p0 / v0 float64 device
    tensors [m, K, 2] -> (pos float64 [m, T, K, 2], valid int32 [m]).
    ``pos`` / ``valid``: write into these contiguous tensors of that shape."""
    import torch
    from paig_reproduction_amd._lib import PaigError, lib, require_device, stream_handle
    require_device(p0)
    require_device(v0)
    q = task_params(task, radius)
    m, K = int(p0.shape[0]), q["K"]
    if not (p0.dtype == torch.float64 and v0.dtype == torch.float64 and tuple(p0.shape) == (m, K, 2) and
            tuple(v0.shape) == (m, K, 2) and p0.is_contiguous() and v0.is_contiguous() and p0.device == v0.device):
        raise PaigError(f"integrate_device: p0 / v0 must be contiguous float64 [m, {K}, 2] on one device")
    pos = torch.empty((m, int(T), K, 2), dtype=torch.float64, device=p0.device) if pos is None else pos
    valid = torch.empty((m,), dtype=torch.int32, device=p0.device) if valid is None else valid
    if not (pos.dtype == torch.float64 and tuple(pos.shape) == (m, int(T), K, 2) and pos.is_contiguous() and
            valid.dtype == torch.int32 and tuple(valid.shape) == (m,) and valid.is_contiguous() and
            pos.device == p0.device and valid.device == p0.device):
        raise PaigError(f"integrate_device: pos must be float64 [m, {int(T)}, {K}, 2] and valid int32 [m] on {p0.device}")
    with torch.cuda.device(p0.device):
        lib().paig_synth_integrate(PHYS_ID[q["phys"]], p0.data_ptr(), v0.data_ptr(), m, K, int(T), q["sub"], q["dt"],
                                   float(q["size"]), float(q["bound"]), q["c0"], q["c1"], pos.data_ptr(),
                                   valid.data_ptr(), stream_handle(p0.device))
    return pos, valid


def draw_device(task, seed, stream, round, m, device=None, radius=2.0, p0=None, v0=None, uniforms=None):
    """``paig_synth_draw`` on the current stream: (p0, v0) float64 device
    tensors [m, K, 2] (``initial_conditions_philox`` is the host twin).
    ``p0`` / ``v0`` / ``uniforms`` (float64 [m, 8]): write into these."""
    import torch
    from paig_reproduction_amd._lib import PaigError, lib, ptr, stream_handle
    q = task_params(task, radius)
    m, K = int(m), q["K"]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    p0 = torch.empty((m, K, 2), dtype=torch.float64, device=dev) if p0 is None else p0
    v0 = torch.empty((m, K, 2), dtype=torch.float64, device=dev) if v0 is None else v0
    for t, shp in ((p0, (m, K, 2)), (v0, (m, K, 2)), (uniforms, (m, DRAW_U))):
        if t is not None and not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shp and
                                  t.is_contiguous() and t.device == p0.device):
            raise PaigError(f"draw_device: outputs must be contiguous float64 device tensors, got {tuple(t.shape)}")
    with torch.cuda.device(p0.device):
        lib().paig_synth_draw(PHYS_ID[q["phys"]], int(seed), int(stream), int(round), m, K, int(bool(q.get("half"))),
                              float(q["size"]), float(q["bound"]), float(q["c0"]), float(q["c1"]),
                              float(q.get("vmax", 0.0)), p0.data_ptr(), v0.data_ptr(), ptr(uniforms),
                              stream_handle(p0.device))
    return p0, v0


def background_device(seed, stream, round, out):
    """``paig_synth_background`` on the current stream into ``out``, a
    contiguous float32 device tensor [n, size, size]."""
    import torch
    from paig_reproduction_amd._lib import PaigError, lib, require_device, stream_handle
    require_device(out)
    if not (out.dtype == torch.float32 and out.dim() == 3 and out.shape[1] == out.shape[2] and out.is_contiguous()):
        raise PaigError("background_device: out must be a contiguous float32 [n, size, size] tensor")
    with torch.cuda.device(out.device):
        lib().paig_synth_background(int(seed), int(stream), int(round), int(out.shape[0]), int(out.shape[1]),
                                    out.data_ptr(), stream_handle(out.device))
    return out


def compact_device(valid, n, rows=None, count=None, totals=None):
    """``paig_synth_compact`` on the current stream: ``valid`` int32 device
    tensor [m] -> (rows int64 [n], count int32 [2]); see include/paig_hip.h.
    Nothing is read back."""
    import torch
    from paig_reproduction_amd._lib import PaigError, lib, ptr, require_device, stream_handle
    require_device(valid)
    n, dev = int(n), valid.device
    if not (valid.dtype == torch.int32 and valid.dim() == 1 and valid.is_contiguous()):
        raise PaigError("compact_device: valid must be a contiguous int32 [m] tensor")
    rows = torch.empty((n,), dtype=torch.int64, device=dev) if rows is None else rows
    count = torch.empty((2,), dtype=torch.int32, device=dev) if count is None else count
    for t, dt, k in ((rows, torch.int64, n), (count, torch.int32, 2), (totals, torch.int64, 3)):
        if t is not None and not (t.is_cuda and t.dtype == dt and tuple(t.shape) == (k,) and t.is_contiguous() and
                                  t.device == dev):
            raise PaigError(f"compact_device: rows int64 [{n}], count int32 [2], totals int64 [3] on {dev}")
    with torch.cuda.device(dev):
        lib().paig_synth_compact(valid.data_ptr(), int(valid.shape[0]), rows.data_ptr(), n, count.data_ptr(),
                                 ptr(totals), stream_handle(dev))
    return rows, count


def rasterize_rows_device(pos, size, radius, rows, out, bg=None):
    """``paig_synth_raster_ex`` on the current stream: ``rows`` is a device
    int64 tensor [n] (``compact_device``) that the host neither reads nor
    checks; sequence i of ``out`` (uint8 [n, T, size, size, 3]) is drawn from
    trajectory ``rows[i]`` and left as it is when that is outside [0, m)."""
    import torch
    from paig_reproduction_amd._lib import PaigError, lib, ptr, require_device, stream_handle
    for t in (pos, rows, out):
        require_device(t)
    if not (pos.dtype == torch.float64 and pos.dim() == 4 and pos.shape[3] == 2 and pos.is_contiguous()):
        raise PaigError("rasterize_rows_device: pos must be a contiguous float64 [m, T, K, 2] tensor")
    m, T, K = int(pos.shape[0]), int(pos.shape[1]), int(pos.shape[2])
    n, dev = int(rows.shape[0]), pos.device
    if not (rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous() and rows.device == dev):
        raise PaigError("rasterize_rows_device: rows must be a contiguous int64 [n] device tensor")
    if not (out.dtype == torch.uint8 and tuple(out.shape) == (n, T, size, size, 3) and out.is_contiguous() and
            out.device == dev):
        raise PaigError(f"rasterize_rows_device: out must be a contiguous uint8 [{n}, {T}, {size}, {size}, 3] tensor")
    if bg is not None and not (bg.is_cuda and bg.dtype == torch.float32 and tuple(bg.shape) == (n, size, size) and
                               bg.is_contiguous() and bg.device == dev):
        raise PaigError(f"rasterize_rows_device: bg must be a contiguous float32 [{n}, {size}, {size}] tensor")
    with torch.cuda.device(dev):
        lib().paig_synth_raster_ex(pos.data_ptr(), rows.data_ptr(), m, n, T, K, int(size), float(radius), ptr(bg),
                                   out.data_ptr(), stream_handle(dev))
    return out


def rasterize_device(pos, size, radius, rows=None, bg=None, out=None):
    """``paig_synth_raster`` on the current stream: pos float64 device tensor
    [m, T, K, 2] -> uint8 [n, T, size, size, 3].

    ``rows`` (host int sequence / array, or an int64 tensor; optional): output
    sequence i draws trajectory ``rows[i]`` (n = len(rows), else n = m); the
    values are range-checked on the host.  ``bg`` (optional): float32 device
    tensor [n, size, size].  ``out``: write into this contiguous uint8 tensor."""
    import torch
    from paig_reproduction_amd._lib import PaigError, lib, ptr, require_device, stream_handle
    require_device(pos)
    if not (pos.dtype == torch.float64 and pos.dim() == 4 and pos.shape[3] == 2 and pos.is_contiguous()):
        raise PaigError("rasterize_device: pos must be a contiguous float64 [m, T, K, 2] tensor")
    m, T, K = int(pos.shape[0]), int(pos.shape[1]), int(pos.shape[2])
    dev = pos.device
    rows_d = None
    n = m
    if rows is not None:
        r = rows.detach().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
        r = np.ascontiguousarray(r, dtype=np.int64).reshape(-1)
        if r.size and (r.min() < 0 or r.max() >= m):
            raise PaigError(f"rasterize_device: rows outside [0, {m})")
        n = int(r.size)
        rows_d = torch.from_numpy(r).to(dev, non_blocking=True)
    if bg is not None:
        require_device(bg)
        if not (bg.dtype == torch.float32 and tuple(bg.shape) == (n, size, size) and bg.is_contiguous() and
                bg.device == dev):
            raise PaigError(f"rasterize_device: bg must be a contiguous float32 [{n}, {size}, {size}] tensor")
    if out is None:
        out = torch.empty((n, T, size, size, 3), dtype=torch.uint8, device=dev)
    else:
        require_device(out)
        if not (out.dtype == torch.uint8 and tuple(out.shape) == (n, T, size, size, 3) and out.is_contiguous() and
                out.device == dev):
            raise PaigError(f"rasterize_device: out must be a contiguous uint8 [{n}, {T}, {size}, {size}, 3] tensor")
    with torch.cuda.device(dev):
        lib().paig_synth_raster(pos.data_ptr(), ptr(rows_d), n, T, K, int(size), float(radius), ptr(bg),
                                out.data_ptr(), stream_handle(dev))
    return out


def render_sequences_device(task, n, seq_len, seed=0, radius=2.0, device=None, chunk=4096, return_state=False):
    """Render ``n`` sequences on the GPU -> uint8 device tensor
    [n, seq_len, H, W, 3] (NHWC, the layout of ``synth.render_sequences``).

    Candidates are drawn from ``np.random.default_rng(seed)`` in rounds of
    exactly ``chunk`` (``initial_conditions``), each round integrated on the
    device; the result is the first ``n`` accepted candidates in stream order,
    rounds continuing until ``n`` are accepted.  The chunk size is fixed, so
    the first ``a`` trajectories of an ``n = b > a`` call are those of the
    ``n = a`` call.  A round costs one device-to-host read (its acceptance
    flags); the accepted rows are rasterised in place, without a compaction
    copy.  For ``mnist_spring_color`` every sequence gets the background
    ``clip(U[0, 1) - 0.2, 0, 1)`` from a ``torch.Generator`` on the device
    seeded with ``seed`` (the prefix property covers the trajectories only).

    These are NOT the sequences of ``synth.render_sequences(seed)``: same
    distribution, another RNG stream.  ``return_state=True`` also returns the
    accepted positions (float64 [n, seq_len, K, 2] on the device)."""
    import torch
    q = task_params(task, radius)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n, T, size, K = int(n), int(seq_len), q["size"], q["K"]
    chunk = int(chunk)
    assert n >= 0 and T > 0 and chunk > 0
    out = torch.empty((n, T, size, size, 3), dtype=torch.uint8, device=dev)
    state = torch.empty((n, T, K, 2), dtype=torch.float64, device=dev) if return_state else None
    bg = None
    if task == "mnist_spring_color" and n:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        bg = (torch.rand((n, size, size), generator=gen, device=dev, dtype=torch.float32) - 0.2).clamp_(0.0, 1.0)
    rng = np.random.default_rng(seed)
    done = 0
    with torch.cuda.device(dev):
        while done < n:
            p0, v0 = initial_conditions(task, rng, chunk, radius)
            pos, valid = integrate_device(task, torch.from_numpy(p0).to(dev), torch.from_numpy(v0).to(dev), T, radius)
            rows = np.flatnonzero(valid.cpu().numpy())[:n - done]   # the round's one sync
            if rows.size:
                rasterize_device(pos, size, q["draw"], rows=rows, bg=None if bg is None else bg[done:done + rows.size],
                                 out=out[done:done + rows.size])
                if state is not None:
                    state[done:done + rows.size] = pos[torch.from_numpy(rows).to(dev)]
                done += int(rows.size)
    return (out, state) if return_state else out


def device_iterators(task, seq_len, n_train, n_valid, n_test, seed, device, rank=0, world=1, data_seed=0):
    """Train / valid / test ``DeviceDataIterator``s over datasets rendered on
    ``device``, never leaving it (no npz).

    Seeds follow ``write_dataset`` and ``get_iterators``: the three splits are
    rendered from ``data_seed``, ``data_seed + 1``, ``data_seed + 2`` and
    shuffled with ``seed``, ``seed + 1``, ``seed + 2`` (``seed=None``: unseeded
    shuffles).  Under data parallelism every rank renders the same dataset and
    takes its shard of each epoch's shared permutation."""
    from .iterators import DeviceDataIterator
    _, size, _ = TASKS[task]
    shape = (int(seq_len), 3, size, size)   # Q5: the NHWC bytes reinterpreted as [C, H, W]

    def mk(n, k):
        x = render_sequences_device(task, n, seq_len, seed=data_seed + k, device=device)
        return DeviceDataIterator(x, shape, device, seed=None if seed is None else seed + k, rank=rank, world=world)

    return mk(n_train, 0), mk(n_valid, 1), mk(n_test, 2)


def streaming_iterators(task, seq_len, batch_size, n_train, n_valid, n_test, seed, device, rank=0, world=1,
                        data_seed=0, stream=True):
    """A ``StreamingDeviceIterator`` for training (nominal epoch ``n_train``;
    every rank streams its own data: the rank is in the Philox key) and
    resident valid / test ``DeviceDataIterator``s rendered once as
    ``device_iterators`` renders them.  No file is read or written.
    ``stream=False`` (a pass that never trains): no training iterator, None."""
    from .iterators import DeviceDataIterator, StreamingDeviceIterator
    _, size, _ = TASKS[task]
    shape = (int(seq_len), 3, size, size)
    train = StreamingDeviceIterator(task, seq_len, batch_size, device, n_train, seed=data_seed if seed is None else seed,
                                    rank=rank, world=world) if stream else None

    def mk(n, k):
        x = render_sequences_device(task, n, seq_len, seed=data_seed + k, device=device)
        return DeviceDataIterator(x, shape, device, seed=None if seed is None else seed + k, rank=rank, world=world)

    return train, mk(n_valid, 1), mk(n_test, 2)
