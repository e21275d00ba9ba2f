"""Host references shared by the synth_device tests (no GPU needed)."""
import numpy as np

from paig_reproduction_amd.nn.datasets import synth
from paig_reproduction_amd.nn.datasets import synth_device as SD

ENVELOPE = 16.0     # device-vs-host64 bound in units of the host64-vs-longdouble spread
FLOOR = 1e-12       # px; below this the spread says nothing


def host_frames(pos, radius, size, bg=None):
    """The composition of synth.render_sequences:126-134 for one sequence:
    pos [T, K, 2] -> uint8 [T, size, size, 3]; bg: float32 [size, size]."""
    T, K, _ = pos.shape
    cov = synth._disk_frames(pos, radius, size)
    frame = np.zeros((T, size, size, 3), dtype=np.float32)
    if bg is not None:
        frame[:] = bg[None, :, :, None]
    for j in range(K):
        ch = 2 - (j % 3)
        frame[..., ch] = np.maximum(frame[..., ch], cov[:, j])
    return (np.clip(frame, 0.0, 1.0) * 255).astype(np.uint8)


def host_envelope(task, p0, v0, T, radius=2.0):
    """float64 and longdouble integrations of the same initial states ->
    (pos64 [m, T, K, 2], valid [m], tol [m], margin [m]).

    tol: the per-sequence bound on |device - pos64|, ENVELOPE times the
    sequence's own float64-vs-longdouble spread (floor FLOOR).  margin: the
    smallest distance of a state the acceptance rule looks at to the frame
    bound it is compared with; an acceptance flag is decided by rounding only
    where margin < tol."""
    q = SD.task_params(task, radius)
    # the spring rule reads the state after every step: for the margin,
    # integrate one more recorded state than the T that are compared
    valid = SD.integrate_host(task, p0, v0, T, radius)[1]
    p64, _ = SD.integrate_host(task, p0, v0, T + 1, radius)
    pld, _ = SD.integrate_host(task, p0, v0, T + 1, radius, dtype=np.longdouble)
    spread = np.abs(p64[:, :T].astype(np.longdouble) - pld[:, :T]).max(axis=(1, 2, 3)).astype(np.float64)
    tol = np.maximum(FLOOR, ENVELOPE * spread)
    lo, hi = q["bound"], q["size"] - q["bound"]
    looked = p64[:, 1:T + 1] if q["phys"] == "spring" else p64[:, :T]
    margin = np.minimum(np.abs(looked - lo), np.abs(looked - hi)).min(axis=(1, 2, 3))
    if q["phys"] == "bounce":
        margin = np.full(len(tol), np.inf)     # accepts everything
    return p64[:, :T], valid, tol, margin


def host_select(task, n, T, seed, chunk, radius=2.0):
    """What render_sequences_device promises: candidates from default_rng(seed)
    in rounds of ``chunk``, the first n accepted in stream order ->
    (pos64 [n, T, K, 2], tol [n], slack, candidates drawn).  slack: the
    smallest margin - tol over every candidate drawn; positive means that no
    acceptance flag, hence no selected row, hangs on rounding."""
    rng = np.random.default_rng(seed)
    pos, tol, slack, drawn = [], [], np.inf, 0
    while sum(len(p) for p in pos) < n:
        p0, v0 = SD.initial_conditions(task, rng, chunk, radius)
        p64, valid, t, margin = host_envelope(task, p0, v0, T, radius)
        drawn += chunk
        slack = min(slack, float((margin - t).min()))
        pos.append(p64[valid])
        tol.append(t[valid])
    return np.concatenate(pos)[:n], np.concatenate(tol)[:n], slack, drawn
