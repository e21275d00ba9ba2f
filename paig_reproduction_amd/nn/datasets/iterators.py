"""Dataset iterators (reference nn/datasets/iterators.py:4-69).

Same semantics: unseeded shuffle per epoch (an optional ``seed`` makes it
reproducible), drop-last (the epoch ends when ``start + batch > N``), uint8/255
to float32, and quirk Q5 — NHWC frames are RESHAPED (not transposed) to
[C, H, W].  ``--datapoints`` is a no-op exactly as in the reference (Q7).

Data-parallel: ``rank``/``world`` give each rank a disjoint slice of every
epoch's shared permutation (a shared ``seed`` keeps the permutations equal).

``DeviceDataIterator`` keeps the dataset in HBM as uint8 and
gathers each batch on the GPU (one HIP launch, /255 fused): same RNG draws,
same batches, no per-step host gather or H2D copy of frames.
"""
import numpy as np


class DataIterator:
    def __init__(self, X, Y=None, seed=None, rank=0, world=1):
        self.X = X
        self.Y = Y
        self.num_examples = self.X.shape[0]
        self.epochs_completed = 0
        self.indices = np.arange(self.num_examples)
        self.rng = np.random.default_rng(seed) if seed is not None else None
        self.rank, self.world = rank, world
        self.reset_iteration()

    def reset_iteration(self):
        if self.rng is not None:
            self.rng.shuffle(self.indices)
        else:
            np.random.shuffle(self.indices)
        self.start_idx = 0

    def get_epoch(self):
        return self.epochs_completed

    def reset_epoch(self):
        self.reset_iteration()
        self.epochs_completed = 0

    def _take(self, batch_size):
        """This rank's indices of the next global batch; drop-last epoch end."""
        gb = batch_size * self.world
        lo = self.start_idx + self.rank * batch_size
        idx = self.indices[lo:lo + batch_size].copy()
        self.start_idx += gb
        if self.start_idx + gb > self.num_examples:
            self.reset_iteration()
            self.epochs_completed += 1
        return idx

    def next_batch(self, batch_size, data_type="train", shuffle=True):
        assert data_type in ["train", "val", "test"], "data_type must be 'train', 'val', or 'test'."
        idx = self._take(batch_size)
        batch_x = self.X[idx]
        batch_y = self.Y[idx] if self.Y is not None else self.Y
        return (batch_x, batch_y)

    def sample_random_batch(self, batch_size):
        # reference quirk kept: the drawn start_idx is unused (iterators.py:42-47)
        np.random.randint(0, self.num_examples - batch_size)
        batch_x = self.X[self.start_idx:self.start_idx + batch_size]
        batch_y = self.Y[self.start_idx:self.start_idx + batch_size] if self.Y is not None else self.Y
        return (batch_x, batch_y)


class DeviceDataIterator(DataIterator):
    """DataIterator over a uint8 dataset resident on ``device``.

    ``X_u8``: uint8 [N, T, H, W, C] (the npz layout); ``shape``: the per-example
    model shape the bytes are reinterpreted as (Q5: (T, C, H, W)).
    next_batch returns a float32 device tensor [B, *shape] gathered by
    paig_gather_u8_f32; ``X`` is the device uint8 tensor (``X.shape[0]`` is N).

    The epoch permutation is drawn on the host exactly as DataIterator draws it
    (same RNG calls, same batches) and uploaded once per epoch; a batch is then
    a slice of that device permutation, so a step issues no host-to-device
    copy at all, only the gather launch.  ``out`` (next_batch / gather_into)
    lets a caller gather into a fixed buffer, e.g. the input of a captured
    HIP graph.

    bind_targets(xbuf, head_frames) makes the decoders read their targets as
    the dataset's bytes (ByteTargets): gathers into xbuf then convert only the
    first head_frames frames of every sequence (the encoder's input) and
    record the batch's dataset rows for the decoders."""

    def __init__(self, X_u8, shape, device, seed=None, rank=0, world=1):
        import torch
        self.shape = tuple(int(d) for d in shape)
        self.row = int(np.prod(X_u8.shape[1:]))
        assert self.row == int(np.prod(self.shape)), (X_u8.shape, shape)
        self.device = torch.device(device)
        self.idx_d = None
        self.bound = None
        if torch.is_tensor(X_u8):
            # a dataset produced on the device (synth_device.py): used as is
            assert X_u8.dtype == torch.uint8 and X_u8.is_contiguous() and X_u8.device == self.device, \
                (X_u8.dtype, X_u8.device, self.device)
            X = X_u8
        else:
            X = torch.from_numpy(np.ascontiguousarray(X_u8)).to(self.device)
        super().__init__(X, None, seed, rank, world)

    def reset_iteration(self):
        import torch
        super().reset_iteration()
        # stream-ordered upload of this epoch's permutation (gathers of the
        # previous epoch that are still queued read their own buffer)
        self.idx_d = torch.from_numpy(self.indices.astype(np.int64)).pin_memory().to(self.device, non_blocking=True)

    def bind_targets(self, xbuf, head_frames):
        """Bind the fixed input buffer ``xbuf`` [B, *shape]: see ByteTargets.
        Returns the binding for ``Engine.byte_targets``."""
        self.bound = ByteTargets(self, xbuf, head_frames)
        return self.bound

    def _launch(self, idx_ptr, n, out):
        from paig_reproduction_amd._lib import lib, stream_handle
        if n:
            bt = self.bound
            if bt is not None and out.data_ptr() == bt.x_ptr:
                assert n == bt.B, (n, bt.B)
                lib().paig_gather_u8_f32_ex(self.X.data_ptr(), idx_ptr, out.data_ptr(), int(n), self.row, bt.head,
                                            bt.idx.data_ptr(), stream_handle(self.device))
            else:
                lib().paig_gather_u8_f32(self.X.data_ptr(), idx_ptr, out.data_ptr(), int(n), self.row,
                                         stream_handle(self.device))
        return out

    def _out(self, n, out):
        import torch
        if out is None:
            return torch.empty((n,) + self.shape, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (n,) + self.shape, \
            (tuple(out.shape), out.dtype)
        return out

    def _gather(self, idx, out=None):
        """Rows ``idx`` (host indices) -> float32 [len(idx), *shape]."""
        import torch
        idx = np.asarray(idx, dtype=np.int64)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < self.num_examples)
        out = self._out(idx.size, out)
        if idx.size:
            idx_d = torch.from_numpy(idx).pin_memory().to(self.device, non_blocking=True)
            self._launch(idx_d.data_ptr(), idx.size, out)
        return out

    def next_batch(self, batch_size, data_type="train", shuffle=True, out=None):
        assert data_type in ["train", "val", "test"], "data_type must be 'train', 'val', or 'test'."
        # the same bookkeeping as DataIterator._take, on the device permutation
        lo = self.start_idx + self.rank * batch_size
        n = max(0, min(batch_size, self.num_examples - lo))
        idx_d = self.idx_d
        out = self._out(n, out)
        self._launch(idx_d.data_ptr() + 8 * lo, n, out)
        self._take(batch_size)   # advances start_idx / epoch (may upload the next permutation)
        return out, None

    def sample_random_batch(self, batch_size):
        np.random.randint(0, self.num_examples - batch_size)   # reference quirk (iterators.py:42-47)
        return self._gather(np.arange(self.start_idx, min(self.start_idx + batch_size, self.num_examples))), None


class StreamPlan:
    """The schedule of ``StreamingDeviceIterator``, without a GPU: which
    events to record and wait on and which half to refill with which batch at
    every ``next_batch`` call, as data.

    The pool has ``depth`` halves of ``B`` slots; batch k lives in half
    k % depth.  ``start()`` is the construction (batches 0 .. depth - 1 filled
    synchronously).  Call number k of ``next(batch_size)`` returns, in issue
    order:

      ("record", "done", k - 1)        compute stream: step k - 1 has ended   (k >= 1)
      ("refill", half, batch, ("done", k - 1))
                                       refill stream: wait for that event, then
                                       write batch k - 1 + depth into half
                                       (k - 1) % depth and record its "filled"
                                       event -- under step k                  (k >= 1)
      ("wait", "filled", half, k)      compute stream: batch k is in half k % depth
      ("gather", half, k)              compute stream: the gather launch

    so a half is rewritten only after the step that read it, and read only
    after the refill that wrote it.  Epochs are nominal: ``epochs_completed``
    advances every ``epoch_size // (B * world)`` batches."""

    def __init__(self, depth, B, epoch_size, world=1):
        self.depth, self.B, self.world = int(depth), int(B), int(world)
        if self.depth < 1 or self.B < 1 or self.world < 1:
            raise ValueError(f"StreamPlan: depth={depth} B={B} world={world}")
        self.epoch_batches = int(epoch_size) // (self.B * self.world)
        if self.epoch_batches < 1:
            raise ValueError(f"StreamPlan: epoch_size={epoch_size} holds no batch of {self.B} x {self.world} ranks")
        self.k = 0                  # next_batch calls so far
        self.in_epoch = 0
        self.epochs_completed = 0

    def start(self):
        return [("fill", j % self.depth, j) for j in range(self.depth)]

    def next(self, batch_size):
        if int(batch_size) != self.B:
            raise ValueError(f"a streaming iterator serves batches of {self.B} only, not {batch_size}")
        k, d = self.k, self.depth
        ops = []
        if k >= 1:
            ops.append(("record", "done", k - 1))
            ops.append(("refill", (k - 1) % d, k - 1 + d, ("done", k - 1)))
        ops.append(("wait", "filled", k % d, k))
        ops.append(("gather", k % d, k))
        self.k += 1
        self.in_epoch += 1
        if self.in_epoch == self.epoch_batches:
            self.in_epoch = 0
            self.epochs_completed += 1
        return ops

    def reset_epoch(self):
        self.in_epoch = 0
        self.epochs_completed = 0


class StreamingDeviceIterator(DeviceDataIterator):
    """An unlimited, never-repeating training stream rendered on the device
    (csrc/synth.hip), living in ``depth`` batches of HBM.

    ``X`` is the pool, uint8 [depth * B, T, H, W, 3]; batch k is read from
    slots (k % depth) * B .. through a persistent device index tensor, by the
    gather of ``DeviceDataIterator`` (``bind_targets`` / ``ByteTargets`` work
    unchanged: the decoders read the pool's rows).  While step k runs, the
    half that step k - 1 read is refilled with batch k - 1 + depth on a stream
    of the iterator's own (``StreamPlan``): draw (``paig_synth_draw``, Philox
    key (seed, rank), round = the batch number) -> integrate -> compact ->
    raster, all into buffers allocated here once.  A refill allocates nothing,
    synchronises nothing and reads nothing back; the host's work per batch is
    the launches.  The stream is a function of (task, seq_len, B, candidates,
    seed, rank) alone.

    Shortfall: a refill that accepts fewer than B of its ``candidates`` writes
    the slots it has rows for; the others keep their previous, still valid
    sequence.  The device counts such slots; ``stats()`` (which synchronises)
    reads the counters.  ``candidates`` defaults to
    ``synth_device.default_candidates`` (expected accepted >= 1.5 B).

    Lifetime: batch k -- the gathered floats' source and, with byte targets
    bound, the pool rows the decoders of the step read -- stays valid until
    the ``next_batch`` call after the one that returned it: that call orders
    the refill of batch k's half after everything queued before it on the
    stream that is current then.  So a step must be queued on that stream
    before the next ``next_batch`` call, and a caller that reads a half after
    its next ``next_batch`` call is unsupported (it may see the next batch's
    bytes).  Refills are never captured into a graph, and none runs during
    ``GraphStep.capture()``: they are issued by ``next_batch`` only, and the
    capture synchronises the device first.  ``num_examples`` is the nominal
    epoch size; ``next_batch`` with any batch size other than B raises."""

    TOPUP_ROUND0 = 1 << 31   # the Philox rounds of construction top-ups: batch numbers stay below

    def __init__(self, task, seq_len, batch_size, device, epoch_size, seed=0, rank=0, world=1, depth=2,
                 candidates=None, radius=2.0):
        import torch
        from . import synth_device as S
        q = S.task_params(task, radius)
        self.task, self.q, self.radius = task, q, radius
        self.B, self.T, self.depth = int(batch_size), int(seq_len), int(depth)
        size, K = q["size"], q["K"]
        self.plan = StreamPlan(self.depth, self.B, epoch_size, world)
        self.key = (int(0 if seed is None else seed), int(rank))
        self.candidates = int(candidates) if candidates else S.default_candidates(task, self.T, self.B, radius=radius)
        dev = torch.device(device)
        X = torch.zeros((self.depth * self.B, self.T, size, size, 3), dtype=torch.uint8, device=dev)
        super().__init__(X, (self.T, 3, size, size), dev, seed=seed, rank=rank, world=world)
        self.num_examples = int(epoch_size)
        m = self.candidates
        f64 = dict(dtype=torch.float64, device=dev)
        self.p0, self.v0 = torch.empty((m, K, 2), **f64), torch.empty((m, K, 2), **f64)
        self.pos = torch.empty((m, self.T, K, 2), **f64)
        self.valid = torch.empty((m,), dtype=torch.int32, device=dev)
        self.rows = torch.empty((self.B,), dtype=torch.int64, device=dev)
        self.count = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.totals = torch.zeros((3,), dtype=torch.int64, device=dev)
        self.bg = torch.empty((self.B, size, size), dtype=torch.float32, device=dev) \
            if task == "mnist_spring_color" else None
        self.refill_stream = torch.cuda.Stream(device=dev)
        self.filled = [torch.cuda.Event() for _ in range(self.depth)]
        self.done = torch.cuda.Event()
        self.construction_rounds = 0
        self._construct()

    def reset_iteration(self):
        # no permutation: the pool's slots in order, uploaded once
        import torch
        if self.idx_d is None:
            self.idx_d = torch.arange(self.X.shape[0], dtype=torch.int64, device=self.device)
        self.start_idx = 0

    def reset_epoch(self):
        self.plan.reset_epoch()
        self.epochs_completed = 0

    def _render(self, round, out, rows, totals):
        """One round on the current stream: candidates of Philox round
        ``round`` -> the accepted ones' frames into ``out`` [n, ...]."""
        from . import synth_device as S
        seed, rank = self.key
        S.draw_device(self.task, seed, rank, round, self.candidates, radius=self.radius, p0=self.p0, v0=self.v0)
        S.integrate_device(self.task, self.p0, self.v0, self.T, self.radius, pos=self.pos, valid=self.valid)
        S.compact_device(self.valid, rows.shape[0], rows=rows, count=self.count, totals=totals)
        bg = None
        if self.bg is not None:
            bg = S.background_device(seed, rank, round, self.bg)[:rows.shape[0]]
        S.rasterize_rows_device(self.pos, self.q["size"], self.q["draw"], rows, out, bg=bg)

    def _construct(self):
        """Fill every slot, synchronously: half h from round h; a half whose
        round accepted fewer than B is topped up from the rounds
        TOPUP_ROUND0, TOPUP_ROUND0 + 1, .. until each slot is written once."""
        import torch
        B, topup = self.B, self.TOPUP_ROUND0
        # the pool and the counters were zeroed on the current stream
        self.refill_stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device), torch.cuda.stream(self.refill_stream):
            for _, h, j in self.plan.start():
                have, round = 0, j
                while have < B:
                    self._render(round, self.X[h * B + have:(h + 1) * B], self.rows[:B - have], None)
                    self.construction_rounds += 1
                    have += int(self.count[0].item())   # construction only: a sync per round
                    round, topup = topup, topup + 1
                self.filled[h].record(self.refill_stream)
        self.refill_stream.synchronize()

    def _refill(self, half, batch):
        import torch
        with torch.cuda.stream(self.refill_stream):
            self._render(batch, self.X[half * self.B:(half + 1) * self.B], self.rows, self.totals)
            self.filled[half].record(self.refill_stream)

    def next_batch(self, batch_size, data_type="train", shuffle=True, out=None):
        import torch
        from paig_reproduction_amd._lib import PaigError
        assert data_type in ["train", "val", "test"], "data_type must be 'train', 'val', or 'test'."
        try:
            ops = self.plan.next(batch_size)
        except ValueError as e:
            raise PaigError(str(e)) from None
        B = self.B
        out = self._out(B, out)
        with torch.cuda.device(self.device):
            compute = torch.cuda.current_stream(self.device)
            for op in ops:
                if op[0] == "record":
                    self.done.record(compute)
                elif op[0] == "refill":
                    self.refill_stream.wait_event(self.done)
                    self._refill(op[1], op[2])
                elif op[0] == "wait":
                    compute.wait_event(self.filled[op[2]])
                else:
                    self._launch(self.idx_d.data_ptr() + 8 * op[1] * B, B, out)
        self.epochs_completed = self.plan.epochs_completed
        return out, None

    def sample_random_batch(self, batch_size):
        from paig_reproduction_amd._lib import PaigError
        raise PaigError("a streaming iterator has no resident dataset to sample from")

    def stats(self):
        """Synchronises the refill stream and reads the device counters:
        refills since construction, the accepted sequences they wrote (mean per
        refill) and the slots they left with their previous sequence."""
        self.refill_stream.synchronize()
        r, acc, short = (int(v) for v in self.totals.cpu().tolist())
        return {"refills": r, "accepted_per_refill": acc / r if r else float("nan"), "shortfall_slots": short,
                "candidates": self.candidates, "construction_rounds": self.construction_rounds}


class ByteTargets:
    """The decoders' targets read from the device-resident dataset (SURVEY §8
    F2 + the fused SSE): a batch gathered into the bound buffer ``xbuf``
    converts only its first ``head_frames`` frames to float32 (what the
    encoder reads; the later frames of xbuf are NOT written), saves the
    batch's dataset rows in ``idx``, and the engine's rollout decoders
    (forward SSE and backward) read frame t of sequence b as X[idx[b]]
    bytes / 255 -- bit-identical to the float32 frame the full gather writes
    (paig_decoder_fwd_t8 / paig_decoder_bwd_t8).  Per sequence of T frames
    this drops the (T - head) float32 frames' write and re-read and reads
    every rollout target at 1 byte a value instead of 4 (the reconstruction
    decoders read the encoder's float32 frames, which are gathered anyway).

    The binding is a promise that only this iterator fills ``xbuf`` (a batch
    written into it otherwise would be decoded against stale rows) and that
    nothing reads its frames >= head_frames (model.input's tail).  The engine
    uses it for an input whose storage is ``xbuf``'s and whose shape matches."""

    SHAPES = ((2, 32), (3, 36), (2, 64))   # (objects, frame side) of the byte-target kernels

    def __init__(self, it, xbuf, head_frames):
        import torch
        assert xbuf.is_contiguous() and xbuf.dtype == torch.float32 and xbuf.device == it.device
        assert tuple(xbuf.shape[1:]) == it.shape, (tuple(xbuf.shape), it.shape)
        self.it = it
        self.B, self.T = int(xbuf.shape[0]), int(it.shape[0])
        self.frame = it.row // self.T
        self.head_frames = int(head_frames)
        assert 0 < self.head_frames <= self.T
        head = self.head_frames * self.frame
        self.head = min(it.row, -(-head // 16) * 16)   # the gather moves 16-byte multiples
        self.x_ptr = xbuf.data_ptr()
        self.base = it.X.data_ptr()
        self.idx = torch.zeros(self.B, dtype=torch.int64, device=it.device)
        self.idx_ptr = self.idx.data_ptr()

    def covers(self, x, lay):
        """True when the engine may decode ``x`` (layout ``lay``) against the
        bytes: x is the bound buffer and the frames it converts cover the
        encoder's."""
        return (x.data_ptr() == self.x_ptr and x.shape[0] == self.B and x.shape[1] == self.T and
                lay.frame == self.frame and lay.Te <= self.head_frames and (lay.K, lay.H) in self.SHAPES)


def get_iterators(file, conv=False, datapoints=0, seed=None, rank=0, world=1, device=None):
    """``device``: keep the uint8 data on that GPU (DeviceDataIterator, F2)."""
    data = np.load(file)
    if conv:
        img_shape = data["train_x"][0, 0].shape
        img_shape = (img_shape[-1], *img_shape[:2])
    else:
        img_shape = data["train_x"][0, 0].flatten().shape

    def mk(key, s):
        x = data[key]
        if device is not None:
            return DeviceDataIterator(x, x.shape[1:2] + img_shape, device, seed=s, rank=rank, world=world)
        return DataIterator(X=x.astype(np.float32).reshape(x.shape[:2] + img_shape) / 255, seed=s, rank=rank,
                            world=world)

    return (mk("train_x", seed), mk("valid_x", None if seed is None else seed + 1),
            mk("test_x", None if seed is None else seed + 2))
