"""Native PhysicsNet step: forward and backward of the reference's training
path, every FLOP in libpaig_hip.so (include/paig_hip.h), orchestrated here.

Reference path: PhysicsNet.conv_feedforward
(nn/network/physics_models.py:204-245) -> compute_loss (:119-142) ->
loss.backward() -> optimizer.step() (nn/network/base.py:141-152).

What is different from the reference, by design (results are the same):
  * the decoder runs ONCE over all B*(Te+R) frames instead of R+1 calls;
    the per-frame SSE of the loss is fused into it;
  * VariableFromNetwork outputs are computed once per step (Q12);
  * the backward is explicit (no autograd graph of ~2k aten nodes): the
    whole step is one autograd.Function whose backward calls the kernels in
    reverse order, writing parameter gradients straight into one flat
    gradient buffer (ready for a single RCCL all-reduce and a fused
    optimizer kernel);
  * the 5-substep physics rollout is one kernel for all R steps.
Nothing here falls back to PyTorch math: torch is used only for device
memory (caching allocator), streams and the autograd hook.
"""
import ctypes
import os
from dataclasses import dataclass, field
from typing import NamedTuple

import torch

from ._lib import PaigError, lib, ptr, stream_handle, require_device
from .decoder_ops import DecoderOps, Sigma, Targets
from .rollout_ops import SPECS, RolloutOps

# The U-Net plans (ShallowUNet blocks.py:240-308, UNet :106-237: buffers,
# ops, which upsamples / pools fuse into which convs, the backward's
# write / accumulate / ReLU' bookkeeping) live in ONE place: csrc/unet.hip,
# whose C-ABI interpreter (paig_unet_fwd_ex / paig_unet_bwd_ex) IS the
# engine's U-Net stage.  Python only names the convs (c1..cN, plan order).


class Switches(NamedTuple):
    """The step's A/B switches (all on by default; "0" turns one off)."""
    fuse_head: bool        # PAIG_FUSE_HEAD: the U-Net's 1x1 head inside the mask softmax (Layout.fuse_head)
    dense_tail: bool       # PAIG_DENSE_TAIL: l2 + position head as fp32 FMA around l1 (Engine.dense_tail)
    fuse_vfn: bool         # PAIG_FUSE_VFN: velocity MLP + VFN sources in one launch
    merge_roll: bool       # PAIG_MERGE_ROLL: rollout + reconstruction decode in one launch
    fused_bwd: bool        # PAIG_FUSED_BWD: the U-Net's fused layer backward
    upt: bool              # PAIG_UPT: upsample backward folded into the conv backward
    pool_fold: bool        # PAIG_POOL_FOLD: max-pool backward folded into the conv backward
    wprep_merge: bool      # PAIG_WPREP_MERGE: weight prep inside the U-Net's first conv launch
    fuse_vel: bool         # PAIG_FUSE_VEL: velocity encoder's input gradient added inside the head backward
    fuse_vfn2: bool        # PAIG_FUSE_VFN2: VFN backward phase 2 inside the head backward's launch
    gemm_epi_merge: bool   # PAIG_GEMM_EPI_MERGE: l2 / l1 weight-gradient epilogues ride in the next GEMM


def read_switches():
    """The one place the step reads its A/B switches from the environment:
    once per forward; the backward uses its own forward's record."""
    return Switches(*[os.environ.get("PAIG_" + f.upper(), "1") != "0" for f in Switches._fields])


class LossAdjoints(NamedTuple):
    """What one compute_loss() backward hands to the decoder backwards: the
    adjoints of (train, extrap, recons), each a 0-d tensor or None, and the
    loss's shape (physics_models._LossReduce)."""
    dt: object
    de: object
    dr: object
    ae: float
    B: int
    Te: int
    R: int
    pred: int


def materialise(adj, mode, dev):
    """The per-frame loss weights of one LossAdjoints as an array (mode 1:
    the B*Te reconstruction frames, 2: the B*R rollout frames)."""
    w = _empty(adj.B * (adj.Te if mode == 1 else adj.R), dev)
    lib().paig_loss_bwd(ptr(adj.dt), ptr(adj.de), ptr(adj.dr), float(adj.ae), ptr(w) if mode == 1 else None,
                        ptr(w) if mode == 2 else None, adj.B, adj.Te, adj.R, adj.pred, stream_handle(dev))
    return w


def live_steps(d_out, d_sse_roll, ent_roll):
    """How many leading rollout steps of every sequence carry a loss weight
    (the rollout decoder backward walks those frames only), or 0 for all of
    them.  Without an extrapolation loss only the first pred steps do
    (physics_models.py:129-139): every loss on this forward's rollout SSE came
    through compute_loss without an extrapolation adjoint (ent_roll: the
    hand-off's (inkernel, LossAdjoints) entries), and nothing else (dense
    frames d_out, the public SSE's d_sse_roll) has a gradient."""
    if d_out is None and d_sse_roll is None and ent_roll and all(adj.de is None for _, adj in ent_roll):
        return ent_roll[0][1].pred
    return 0


class Layout:
    """Static shapes of one step (from the PhysicsNet config and batch)."""

    def __init__(self, model, B, T, sw, frames=None, net=None):
        """sw: the forward's Switches.
        frames=N: the encoder alone over N independent frames (the
        standalone ConvolutionalEncoder / U-Net calls): F = N, no sequence.
        net: "unet" / "shallow_unet" to plan that U-Net whatever the frame
        size (both are built, Q8; the live one is chosen by H otherwise)."""
        self.B, self.T, self.sw = B, T, sw
        self.sequences = frames is None
        self.K = model.n_objs
        self.D = model.coord_units // 2
        self.H = model.conv_input_shape[1]
        self.h = self.H // 2
        self.ins, self.pred = model.input_steps, model.pred_steps
        self.Te = self.ins + self.pred
        self.R = model.pred_steps + model.extrap_steps
        if frames is None:
            assert T == model.seq_len, f"input has {T} frames, model expects seq_len={model.seq_len}"
            self.F = B * self.Te
        else:
            self.F = frames
        self.alt_vel = model.alt_vel
        self.spec = SPECS[model.cell_type]   # the rollout cell's kernels, operands and parameter names
        self.cell = self.spec.kind
        self.unet = self.H >= 40 if net is None else net == "unet"
        L = lib()
        self.net = 1 if self.unet else 0   # paig_unet_*: 0 ShallowUNet(hidden 8), 1 UNet(hidden 16)
        self.prefix = "encoder.unet." if self.unet else "encoder.shallow_unet."
        self.nconv = L.paig_unet_query(self.net, self.K, 0)
        self.lg_relu = not self.unet   # ShallowUNet's c13 output is ReLU'd (Q13), UNet's c18 not
        # l1 input: the masked objects, AvgPool2d(2)'d first for H >= 40 (blocks.py:92-96)
        self.l1_in = 3 * (self.H // 2) ** 2 if self.unet else 3 * self.H * self.H
        self.HW = self.H * self.H
        self.frame = 3 * self.HW
        # output sizes of the VariableFromNetwork sources, in _VFN order
        self.vfn_sizes = (self.K * self.h * self.h, self.K * 3 * self.h * self.h, 3 * self.HW)
        # the U-Net's last layer, a 1x1 head (ShallowUNet c13, 8 -> K, ReLU'd;
        # UNet c18, 16 -> K, with the objects' AvgPool2d), is fused into the
        # mask softmax (paig_head_mask_fwd_ex / _bwd_ex) in the encoder; the
        # standalone U-Net call keeps it as a conv (its logits are the output).
        # PAIG_FUSE_HEAD=0: the separate conv + softmax kernels (A/B)
        self.head_buf = L.paig_unet_query(self.net, self.K, 2)
        self.head_ci = L.paig_unet_query(self.net, self.K, 3)
        self.head_name = f"c{self.nconv}"
        self.head_flags = (1 if self.lg_relu else 0) | (2 if self.unet else 0)
        self.fuse_head = (self.K in (2, 3) and self.HW % 4 == 0 and sw.fuse_head and
                          ((not self.unet and self.head_ci == 8) or (self.unet and self.head_ci == 16 and
                                                                     self.H % 4 == 0)))
        if self.fuse_head:
            # the fused head kernels read the head input (and write its
            # gradient) as [F][head_ci][H][W] from the start of its buffer
            off, cbuf = L.paig_unet_query(self.net, self.K, 5), L.paig_unet_query(self.net, self.K, 6)
            if off != 0 or cbuf != self.head_ci:
                raise PaigError(f"U-Net head input at channel offset {off} of a {cbuf}-channel buffer: the fused "
                                f"head needs the whole buffer ({self.head_ci} channels from offset 0)")


class KernelProbe:
    """Times every launch of one tagged kernel (``tag``), or of every tagged
    kernel (``tag=None``), with HIP events recorded on the step's stream
    (bench.py's roofline numbers)."""

    backlog_cycles = 1 << 20

    def __init__(self, tag):
        self.tag = tag
        self.events = {}
        self.work = {}

    def wrap(self, tag, flops, nbytes=0):
        probe = self
        want = probe.tag is None or tag == probe.tag

        class _Ctx:
            def __enter__(self):
                if want:
                    self.e0 = torch.cuda.Event(enable_timing=True)
                    self.e1 = torch.cuda.Event(enable_timing=True)
                    # a spin kernel first: the stream is then backlogged when the
                    # start event and the probed kernel are enqueued, so the host's
                    # launch latency between them does not count as kernel time
                    torch.cuda._sleep(probe.backlog_cycles)
                    self.e0.record()
                return self

            def __exit__(self, *exc):
                if want:
                    self.e1.record()
                    probe.events.setdefault(tag, []).append((self.e0, self.e1))
                    probe.work[tag] = (flops, nbytes)
                return False

        return _Ctx()

    def overhead_ms(self, n=20):
        """The event pair's own cost around one dispatch: the same bracket
        (backlogged stream, start event, launch, end event) around a spin
        kernel of zero cycles.  Subtracted from the probed intervals so they
        compare with rocprof's kernel start-to-end durations."""
        pairs = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(self.backlog_cycles)
            e0.record()
            torch.cuda._sleep(0)
            e1.record()
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        return min(a.elapsed_time(b) for a, b in pairs)

    def summaries(self):
        """{tag: {tag, n, avg_ms, avg_ms_raw, flops, bytes}} (per launch;
        avg_ms net of the event bracket's overhead)."""
        torch.cuda.synchronize()
        ovh = self.overhead_ms() if self.events else 0.0
        out = {}
        for tag, evs in self.events.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            fl, nb = self.work[tag]
            raw = sum(ms) / len(ms)
            out[tag] = {"tag": tag, "n": len(ms), "avg_ms": max(raw - ovh, 1e-6), "avg_ms_raw": raw,
                        "overhead_ms": ovh, "flops": fl, "bytes": nb}
        return out

    def summary(self):
        s = self.summaries()
        return s.get(self.tag) if self.tag is not None else None


class _NoProbe:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NOPROBE = _NoProbe()


def _parr(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _iarr(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _empty(n, device, dtype=torch.float32):
    return torch.empty(n, device=device, dtype=dtype)


# the VariableFromNetwork sources, in the order of every paig_vfn_*_multi array
_VFN = ("var_net_template", "var_net_content", "var_net_background")
# the head backward's arguments when it carries no velocity term / no VFN phase 2
_NO_VEL = (None, None, 0, 0, 0, 0)
_NO_VFN2 = (0,) + (None,) * 11


@dataclass(slots=True, eq=False)
class StepState:
    """What one forward saves for its backward (Engine.new_state is the only
    constructor).  Every field is declared here: a misspelt one raises."""
    lay: Layout = None          # new_state; every stage
    x: object = None            # new_state: the input (x_view and tgt_roll point into it)
    ws: object = None           # new_state: GEMM workspace of the dense layers; forward and backward
    dev: object = None          # new_state; every stage
    cm: int = 0                 # new_state: conv arithmetic flags; _unet_forward, _unet_grad, _unet_backward
    need_saved: bool = True     # new_state: a backward may follow; _unet_forward (else the inference workspace)
    sw: Switches = None         # new_state: the forward's A/B switches; every stage
    x_view: tuple = None        # new_state: the encoder's frames (pointer, stride, group, group stride)
    sigma: Sigma = None         # forward: the decoders' window scale: model.decoder_sigma(), or (learn_sigma) the
    #                             model's one-double device sigma, written by paig_sigma_from_u at the start of the
    #                             forward; the decoders' forward and backward
    tgt_rec: Targets = None     # forward: the reconstruction decoders' targets (the encoder's frames); backward
    tgt_roll: Targets = None    # forward: the rollout decoders' targets (x's frames or the dataset's bytes); backward
    src: dict = None            # forward: VFN buffers {name: (hidden, raw, post-sigmoid or None)}; backward
    Xv: object = None           # forward: velocity encoder input rows; backward
    v1: object = None           # forward: velocity MLP hidden 1; backward
    v2: object = None           # forward: velocity MLP hidden 2; backward
    vel0: object = None         # forward: initial velocities, None when input_steps == 1; backward
    pvs: object = None          # forward: rollout positions and velocities; backward
    roll_ws: object = None      # forward (a learned cell, a backward may follow): the cell's saved activations; backward
    wprep: dict = None          # _unet_forward: split weight images {(conv, kind): pointer}; _encoder_forward
    wprep_buf: object = None    # _unet_forward: the buffer behind wprep (kept alive)
    logits: object = None       # _unet_forward (head not fused): the U-Net's logits; mask softmax, _unet_backward
    head_in: object = None      # _unet_forward (head fused, else None): the head's input in unet_ws; mask softmax
    unet_ws: object = None      # _unet_forward: the U-Net workspace; _unet_grad, _unet_backward; release drops it
    unet_flags: int = 0         # _unet_forward: paig_unet_*_ex flags; _unet_grad, _unet_backward
    unet_wp: tuple = None       # _unet_forward: (forward, dgrad) weight-image arrays; _unet_backward
    dense_tail: bool = False    # _encoder_forward: l2 + head ran fused; _encoder_backward
    w2t: object = None          # _encoder_forward: W2^T scratch when wprep has none (kept alive)
    masks: object = None        # _encoder_forward; forward's result, _encoder_backward
    objs: object = None         # _encoder_forward; forward's result
    l1_x: object = None         # _encoder_forward: l1's input (the objects, pooled for the UNet); _encoder_backward
    h1: object = None           # _encoder_forward: l1's output; _encoder_backward
    h2: object = None           # _encoder_forward: l2's output; _encoder_backward
    h3: object = None           # _encoder_forward: the position head's pre-activation; _encoder_backward
    enc_pos: object = None      # _encoder_forward; forward's decoders and velocity encoder, backward
    extra_slabs: list = field(default_factory=list)   # backward stages: (slab, rows, len, grad); _unet_backward
    consumed: bool = False      # release; check_fresh
    probe_cb: object = None     # Engine._unet_probe: the ctypes callback, alive as long as the state

    def release(self):
        """Drop the forward's U-Net workspace (activations, gradients, max-|x|
        slots, pool codes) once its backward has been queued, or there is none;
        stream order keeps the allocator's next user behind every kernel that
        reads it.  The state then admits no second backward (retain_graph=True)."""
        self.unet_ws = None
        self.consumed = True

    def check_fresh(self):
        if self.consumed:
            raise PaigError("a second backward through one forward (retain_graph=True) is not supported: the "
                            "forward's saved state (its U-Net workspace) was released by the first backward")


class Engine:
    """Binds a PhysicsNet's parameters to the HIP kernels."""

    def __init__(self, model):
        self.model = model
        self.L = lib()
        self.probe = None
        self.last_masked_objs = None
        self.last_sigma = 1.0           # the last forward's decoder window scale (StepState.sigma.value)
        self.last_loss_handoff = None   # the last forward's loss-weight hand-off (physics_models._LossHandoff)
        # called once per backward when the early gradient bucket is final
        # (FlatParams.allreduce_early by default; bench.py splits its HIP graph here)
        self.bucket_hook = model._flat.allreduce_early
        # DeviceDataIterator.ByteTargets bound to the step's input buffer: the
        # decoders then read their targets as the dataset's bytes
        self.byte_targets = None

    # conv arithmetic (include/paig_hip.h flags): "split" = f16 hi/lo pieces on
    # the 16-bit matrix cores, operands scaled by powers of two (fp32-accurate:
    # within 3x the fp32 reference's own error, tests/test_gpu_envelope.py),
    # "fp32" = f32-input MFMA, "bf16" = bf16 operands (BASELINE config #2)
    CONV_MATH = {"split": 128, "fp32": 0, "bf16": 256}

    # the same choice for the dense layers (paig_gemm_ex math) per GEMM kind
    # (forward, wgrad, dgrad): f16 pieces, both operands (activations /
    # gradients and the weights) scaled by running powers of two (math 6): no
    # range limit on any operand
    GEMM_MATH = {"split": (6, 6, 6), "fp32": (0, 0, 0), "bf16": (3, 3, 3)}
    FWD, WGRAD, DGRAD = 0, 1, 2

    def gemm_math(self, kind):
        return self.GEMM_MATH[getattr(self.model, "conv_math", "split")][kind]

    def conv_flags(self):
        m = getattr(self.model, "conv_math", "split")
        if m not in self.CONV_MATH:
            raise ValueError(f"conv_math must be one of {sorted(self.CONV_MATH)}, got {m!r}")
        return self.CONV_MATH[m]

    @staticmethod
    def _dec_bytes(n, lay, tb=4):
        """Algorithmic HBM bytes of one decoder forward over n frames: the
        target frames read (fused SSE; tb bytes per value: 4 fp32, 1 for the
        dataset's bytes) and the decoded frames written; positions and the
        step-constant sources (< 100 KB) are negligible."""
        return n * lay.frame * (tb + 4)

    @staticmethod
    def _dec_bwd_bytes(live, n, lay, dense, tb=4):
        """Algorithmic HBM bytes of one decoder backward: the targets of the
        `live` frames that carry a loss weight (+ their dense dL/dout when
        given) read, the position gradients of all n frames and the source
        gradients (one slab_len vector) written.  The partial-gradient slab
        rows are the kernel's own overhead, not algorithmic."""
        return (live * lay.frame * (tb + (4 if dense else 0)) + n * 2 * lay.D * 4
                + (4 * lay.K * lay.h * lay.h + 3 * lay.HW) * 4)

    def _p(self, tag, flops=0, nbytes=0):
        """Probe context of one launch: algorithmic FLOPs and HBM bytes (the
        compulsory operand reads + result writes) for bench.py's roofline."""
        if self.probe is None or tag is None:   # (no tag: an unlabelled launch)
            return _NOPROBE
        return self.probe.wrap(tag, flops, nbytes)

    # -- parameter access ------------------------------------------------
    def p(self, name):
        return self.model._param_by_name[name]

    def g(self, name):
        return self.model._flat.grad_view(name)

    # -- small helpers ---------------------------------------------------
    def linear(self, x, rows, name, out, act, st, ws):
        """out[rows, O] = act(x[rows, I] W^T + b) ; W = name.weight [O, I]"""
        W, b = self.p(name + ".weight"), self.p(name + ".bias")
        O, I = W.shape
        with self._p("gemm_fwd:" + name, 2 * rows * O * I, 4 * (rows * I + O * I + rows * O)):
            self.L.paig_gemm_ex(0, 1, rows, O, I, 1.0, ptr(x), I, ptr(W), I, 0.0, ptr(out), O, ptr(b), act, 0, None,
                                0, None, ptr(ws), ws.numel() if ws is not None else 0, self.gemm_math(self.FWD), st)

    def linear_bwd(self, x, dy, rows, name, dx, aux, auxm, st, ws, need_dx=True, defer_epi=False):
        """dW = dy^T x and db = colsum(dy) (one GEMM, fused row sums) ; dx = (dy W) * act'(aux).
        defer_epi: the weight gradient's split-K epilogue rides in the next
        GEMM's launch (paig_gemm_defer_epilogue; the caller flushes)."""
        W = self.p(name + ".weight")
        O, I = W.shape
        gW, gb = self.g(name + ".weight"), self.g(name + ".bias")
        n_ws = ws.numel()
        if defer_epi:
            self.L.paig_gemm_defer_epilogue(1)
        with self._p("gemm_wgrad:" + name, 2 * rows * O * I, 4 * (rows * O + rows * I + O * I + O)):
            self.L.paig_gemm_ex(1, 0, O, I, rows, 1.0, ptr(dy), O, ptr(x), I, 0.0, ptr(gW), I, None, 0, 0, None, 0,
                                ptr(gb), ptr(ws), n_ws, self.gemm_math(self.WGRAD), st)
        if need_dx:
            # dY and W read, dX written (+ the activation read for its derivative)
            with self._p("gemm_dgrad:" + name, 2 * rows * O * I, 4 * (rows * O + O * I + (2 if auxm else 1) * rows * I)):
                self.L.paig_gemm_ex(0, 0, rows, I, O, 1.0, ptr(dy), O, ptr(W), I, 0.0, ptr(dx), I, None, 0, auxm,
                                    ptr(aux), I, None, ptr(ws), n_ws, self.gemm_math(self.DGRAD), st)

    def dense_tail(self, sw):
        """The localiser's l2 + head as fp32 FMA inside the launches around
        them (paig_dense_tail_fwd / paig_head_l2_bwd): in split arithmetic,
        where the 3-MFMA l2 GEMMs were latency-bound launches of their own;
        bf16 keeps its 1-MFMA l2 GEMMs (faster there).  PAIG_DENSE_TAIL=0: A/B."""
        return self.gemm_math(self.FWD) == 6 and sw.dense_tail

    def workspace_floats(self, lay):
        K, F, B = lay.K, lay.F, lay.B
        n1 = lay.l1_in
        need = [self.L.paig_gemm_workspace(K * F, 200, n1), self.L.paig_gemm_workspace(K * F, 200, 200),
                self.L.paig_gemm_workspace(200, n1, K * F), self.L.paig_gemm_workspace(K * F, n1, 200), self.L.paig_gemm_workspace(200, 200, K * F),
                self.L.paig_gemm_workspace(2, 200, K * F), self.L.paig_gemm_workspace(100, 100, K * B),
                # l2's and l1's weight-gradient partials side by side (their epilogues are deferred)
                self.L.paig_gemm_workspace(200, 200, K * F) + self.L.paig_gemm_workspace(200, n1, K * F),
                self.L.paig_gemm_workspace(K * B, 100, 100), 1 << 16,
                self.L.paig_gemm_parts_size(K * F, 200, n1, self.gemm_math(self.FWD))]
        return int(max(need))

    # -- argument packs (each built in one place, splatted at every call) ----
    def _velmlp_params(self):
        """The velocity MLP's (W0, b0, W2, b2, W4, b4) pointers."""
        pm = "velocity_encoder.init_vel_mlp."
        return tuple(ptr(self.p(pm + n)) for n in ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"))

    def _vfn_fwd_args(self, S):
        """paig_vfn_fwd_multi's arrays: (n, W1, b1, W2, b2, hidden, raw, post-sigmoid, sizes)."""
        return (3, *[_parr([ptr(self.p(nm + suf)) for nm in _VFN])
                     for suf in (".l1.weight", ".l1.bias", ".l2.weight", ".l2.bias")],
                *[_parr([ptr(S.src[nm][i]) for nm in _VFN]) for i in range(3)], _iarr(S.lay.vfn_sizes))

    def _vfn_bwd_args(self, S, dsrc, vparts):
        """paig_vfn_bwd*_multi's arrays: (n, d output, raw output, sigmoid?,
        hidden, W2, dW1, db1, dW2, db2, block partials, sizes); dsrc = [d
        template | d sigmoid(content) | d sigmoid(background)]."""
        P = S.lay.vfn_sizes
        return (3, _parr([ptr(dsrc) + o * 4 for o in (0, P[0], P[0] + P[1])]),
                _parr([ptr(S.src[nm][1]) for nm in _VFN]), _iarr([0, 1, 1]),
                _parr([ptr(S.src[nm][0]) for nm in _VFN]), _parr([ptr(self.p(nm + ".l2.weight")) for nm in _VFN]),
                *[_parr([ptr(self.g(nm + suf)) for nm in _VFN])
                  for suf in (".l1.weight", ".l1.bias", ".l2.weight", ".l2.bias")],
                _parr([ptr(pt) for pt in vparts]), _iarr(P))

    def _rollout_ops(self, lay):
        """The rollout calls of the model's cell at this step's shape."""
        return RolloutOps(self.L, self.model.rollout_cell, lay.B, lay.D, lay.R, float(lay.H / 2))

    def _decoder_ops(self, S):
        """The decoder calls of this forward's sigma and VFN sources."""
        lay = S.lay
        return DecoderOps(self.L, lay.K, lay.h, lay.H, S.sigma, (ptr(S.src["var_net_template"][1]),
                                                                 ptr(S.src["var_net_content"][1]),
                                                                 ptr(S.src["var_net_background"][2])))

    @staticmethod
    def _roll_pos(S):
        """The rollout frames' position view: steps 1..R of every sequence of pvs."""
        D, R = S.lay.D, S.lay.R
        return (ptr(S.pvs) + 2 * D * 4, (R + 1) * 2 * D, 2 * D, R)

    def _head_bwd_prefix(self, S, denc, dh2, hslab):
        """(h2, h3, d enc_pos, W3, d h2, slab, F, K, 200, H/2) of every paig_head*_bwd* entry point."""
        lay = S.lay
        return (ptr(S.h2), ptr(S.h3), ptr(denc), ptr(self.p("encoder.l3.weight")), ptr(dh2), ptr(hslab), lay.F, lay.K,
                200, float(lay.H / 2))

    # -- forward ---------------------------------------------------------
    def new_state(self, lay, x, need_saved):
        """The saved state of one forward over x (contiguous fp32): the
        layout's switches, the dense layers' workspace and the view of the
        encoder's frames (frame n = b*Te + t of x's sequences, or x's own
        frames for the standalone encoder / U-Net calls)."""
        S = StepState()
        S.lay, S.x, S.need_saved, S.sw = lay, x, need_saved, lay.sw
        S.dev = x.device
        S.cm = self.conv_flags()
        S.ws = _empty(self.workspace_floats(lay), S.dev)
        S.x_view = (ptr(x), lay.T * lay.frame, lay.Te, lay.frame) if lay.sequences else (ptr(x), lay.frame, 0, 0)
        return S

    def forward(self, x, need_saved=True, grad_mode=True):
        require_device(x)
        model = self.model
        model._flat.ensure()
        B, T = x.shape[0], x.shape[1]
        lay = Layout(model, B, T, read_switches())
        L = self.L
        x = x.contiguous()
        learn = getattr(model, "learn_sigma", False)
        # log_sig is read at every forward, as in the reference; the learnable
        # scale is never read by the host (decoder_sigma() would synchronise)
        S = self.new_state(lay, x, need_saved)
        S.sigma = Sigma(model.sigma_buffer() if learn else model.decoder_sigma())
        dev, ws, sw = S.dev, S.ws, S.sw
        st = stream_handle(dev)
        if learn:   # sigma from u, on the step's stream: captured with the graph
            L.paig_sigma_from_u(ptr(self.p("decoder_sigma_u")), S.sigma.arg, st)
        self.last_sigma = S.sigma.value
        K, F, HW, H, h, D = lay.K, lay.F, lay.HW, lay.H, lay.h, lay.D

        # ---- VariableFromNetwork sources (once per step, Q12; only the decoders read them)
        S.src = {nm: (_empty(200, dev), _empty(P, dev), _empty(P, dev) if nm == "var_net_background" else None)
                 for nm, P in zip(_VFN, lay.vfn_sizes)}
        tmpl, cont, bgp = S.src["var_net_template"][1], S.src["var_net_content"][1], S.src["var_net_background"][2]

        # ---- encoder over the first Te frames of every sequence (in place)
        # the rollout decoders' targets: x's frames, or (byte targets bound to
        # this input buffer) the dataset rows it was gathered from, as bytes.
        # The reconstruction targets are the encoder's frames, which the
        # gather writes as fp32 in either case: read there (no row lookup)
        bt = self.byte_targets
        if bt is not None and bt.covers(x, lay):
            S.tgt_roll = Targets.dataset_bytes(bt.base + lay.ins * lay.frame, bt.idx_ptr, T * lay.frame, lay.R,
                                               lay.frame)
        else:
            S.tgt_roll = Targets.frames(ptr(x) + lay.ins * lay.frame * 4, T * lay.frame, lay.R, lay.frame)
        S.tgt_rec = Targets.frames(*S.x_view)
        self._encoder_forward(S, st)
        enc_pos = S.enc_pos

        # Two independent chains follow the position head: velocity MLP ->
        # physics rollout (one thread per sequence: latency-bound, a few
        # blocks) and VFN sources -> reconstruction decode of all B*Te frames.
        # They share the step's one stream, merged into common launches where
        # the shape allows.
        recons = _empty(F * lay.frame, dev)
        sse_rec = _empty(F, dev)
        if lay.ins > 1:
            S.Xv = _empty(K * B * 2 * (lay.ins - 1 if lay.alt_vel else lay.ins), dev)
            S.vel0 = _empty(K * B * 2, dev)
            if not lay.alt_vel:
                S.v1 = _empty(K * B * 100, dev)
                S.v2 = _empty(K * B * 100, dev)
        S.pvs = _empty(B * (lay.R + 1) * 2 * D, dev)
        rops = self._rollout_ops(lay)
        if lay.spec.saves(need_saved, grad_mode):
            S.roll_ws = _empty(rops.workspace_floats(), dev)
        # (pos0, ld, vel0, pvs): the rollout starts at the last input step's encoded positions
        roll = (ptr(enc_pos) + (lay.ins - 1) * D * 4, lay.Te * D, ptr(S.vel0), ptr(S.pvs))
        vel_act = (ptr(S.Xv), ptr(S.v1), ptr(S.v2), ptr(S.vel0))
        dec = self._decoder_ops(S)
        # velocity MLP + VFN sources in one launch (independent); then the
        # rollout and the reconstruction decode in one launch
        fuse_vfn = S.vel0 is not None and not lay.alt_vel and sw.fuse_vfn
        merge_roll = fuse_vfn and self._merge_roll_rec(lay)
        if fuse_vfn:
            L.paig_velmlp_vfn_fwd(ptr(enc_pos), B, lay.Te, K, lay.ins, *self._velmlp_params(), *vel_act,
                                  *self._vfn_fwd_args(S), st)
        elif S.vel0 is not None and lay.alt_vel:
            L.paig_vel_pack(ptr(enc_pos), ptr(S.Xv), B, lay.Te, K, lay.ins, 1, st)
            self.linear(S.Xv, K * B, "velocity_encoder.init_vel_linear", S.vel0, 0, st, ws)
        elif S.vel0 is not None:   # the whole MLP (packing fused) in one launch
            L.paig_velmlp_fwd(ptr(enc_pos), B, lay.Te, K, lay.ins, *self._velmlp_params(), *vel_act, st)
        if not merge_roll:   # all R steps in one launch (a learned cell never merges: _ROLL_REC has none)
            with self._p(lay.spec.family.probe_fwd):
                rops.fwd(*roll, S.roll_ws, st)
        if not fuse_vfn:
            L.paig_vfn_fwd_multi(*self._vfn_fwd_args(S), st)
        # reconstruction decode (all B*Te frames, SSE vs input fused)
        with self._p("dec_fwd:recon+rollout" if merge_roll else "dec_fwd:recon", 0, self._dec_bytes(F, lay)):
            dec.fwd((ptr(enc_pos), 0, 2 * K, 0), ptr(recons), lay.frame, S.tgt_rec, ptr(sse_rec), F, st,
                    roll=rops.merged_args(*roll) if merge_roll else None)

        # ---- rollout decode (all B*R frames in one launch, SSE vs input[:, ins:])
        out = _empty(B * lay.R * lay.frame, dev)
        sse_roll = _empty(B * lay.R, dev)
        with self._p("dec_fwd:rollout", 0, self._dec_bytes(B * lay.R, lay, S.tgt_roll.value_bytes)):
            dec.fwd(self._roll_pos(S), ptr(out), lay.frame, S.tgt_roll, ptr(sse_roll), B * lay.R, st)

        masks, objs = S.masks, S.objs
        res = {
            "output_seq": out.view(B, lay.R, 3, H, H),
            "recons_out": recons.view(B, lay.Te, 3, H, H),
            "enc_pos": enc_pos.view(B, lay.Te, D),
            "pos_vel_seq": S.pvs.view(B, lay.R + 1, 2 * D),
            "enc_masks": masks.view(F, K + 1, H, H),
            "masked_objs": [objs[k * F * 3 * HW:(k + 1) * F * 3 * HW].view(F, 3, H, H) for k in range(K)],
            "sse_rec": sse_rec,
            "sse_roll": sse_roll,
            "template": tmpl.view(K, 1, h, h),
            "contents": cont.view(K, 3, h, h),
            "background_content": bgp.view(1, 3, H, H),
        }
        if not need_saved:
            S.release()
        return res, (S if need_saved else None)

    # (K, H, cell) of paig_decoder_fwd_rollout (the one-CU decoder's shapes)
    # -> threads per block (DecFw<K, H>::NT: one rollout sequence per thread)
    _ROLL_REC = {(2, 32, 0): 256, (2, 32, 1): 256, (3, 36, 2): 384, (2, 64, 0): 1024}

    def _merge_roll_rec(self, lay):
        """The rollout and the reconstruction decode share one launch while
        the decode's blocks leave room for the rollout's in one round of four
        blocks per CU (B=100: 500 + 1 blocks; B >= 512 measured 0.4-0.6%
        slower merged).  PAIG_MERGE_ROLL=0: two launches (the A/B)."""
        nt = self._ROLL_REC.get((lay.K, lay.H, lay.cell))
        if nt is None or not lay.sw.merge_roll:
            return False
        return min((lay.F + 1) // 2, 1024) + -(-lay.B // nt) <= 1024

    # probe kinds of paig_unet_*_ex (include/paig_hip.h PAIG_PROBE_*) -> tag prefix
    _PROBE_TAG = {0: "conv_fwd", 1: "conv_bwd", 2: "conv_wgrad", 3: "conv_dgrad"}
    _PROBE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int)

    def _unet_probe(self, S):
        """The per-launch probe callback of the C U-Net interpreter: HIP
        events around every conv launch (KernelProbe) with its algorithmic
        FLOPs and HBM bytes (bench.py's roofline); None when not probing."""
        if self.probe is None:
            return None
        lay, F = S.lay, S.lay.F
        open_ = {}

        def cb(ctx, ev, op, conv, kind, cin, cout, Hl, fl):
            if ev == 1:
                open_.pop(op).__exit__(None, None, None)
                return
            ks = self.p(lay.prefix + f"c{conv + 1}.weight").shape[-1]
            flops = 2 * F * cin * cout * ks * ks * Hl * Hl
            up = bool(fl & 32)
            hin = Hl // 2 if up else Hl
            if kind == 0 or kind == 2:     # forward / weight gradient: X and Y (dY) once
                nbytes = 4 * F * (cin * hin * hin + cout * Hl * Hl)
            elif kind == 1:                # fused layer backward: data + weight gradients
                flops *= 2
                if up:   # the half-resolution source (and its ReLU' mask) and dY read, its gradient written
                    nbytes = 4 * F * (cin * hin * hin * (2 if fl & 2 else 1) + cout * Hl * Hl)
                else:    # X and dY read, dX written (+ read when accumulating)
                    nbytes = 4 * F * Hl * Hl * (cin + cout + cin * (2 if fl & 4 else 1))
                    if fl & 64:   # the folded max pool: pooled gradient + window codes
                        nbytes += F * (4 * cout + cout) * (Hl // 2) ** 2
            elif fl & 512:                 # data gradient into the upsample source: dY read, its gradient (+ mask)
                nbytes = 4 * F * (cout * Hl * Hl + cin * (Hl // 2) ** 2 * (2 if fl & 2 else 1))
            else:                          # data gradient: dY read, dX written (+ mask, + accumulate)
                nbytes = 4 * F * Hl * Hl * (cout + cin * (1 + (1 if fl & 2 else 0) + (1 if fl & 4 else 0)))
            c = self._p(f"{self._PROBE_TAG[kind]}:c{conv + 1}", flops, nbytes)
            c.__enter__()
            open_[op] = c

        S.probe_cb = self._PROBE_FN(cb)   # alive as long as the saved state
        return ctypes.cast(S.probe_cb, ctypes.c_void_p)

    def _unet_forward(self, S, st, fuse_head=False):
        """The U-Net over the F frames of S.x_view: the C interpreter of
        csrc/unet.hip (paig_unet_fwd_ex) in one workspace that the backward
        reuses.  Leaves the logits (S.logits), or, fuse_head, the 1x1 head's
        input (S.head_in: c12's / c17's output, which the encoder's fused mask
        softmax reads)."""
        L = self.L
        lay, sw, dev, cm = S.lay, S.sw, S.dev, S.cm
        F, H, K = lay.F, lay.H, lay.K
        flags = ((1 if fuse_head else 0) | (0 if S.need_saved else 4) |
                 (0 if sw.fused_bwd else 2) |   # A/B: separate data / weight gradient launches
                 (0 if sw.upt else 16) |        # A/B: standalone upsample backward
                 (0 if sw.pool_fold else 32))   # A/B: standalone pool backward
        Ws = [self.p(lay.prefix + f"c{c + 1}.weight") for c in range(lay.nconv)]
        Bs = [self.p(lay.prefix + f"c{c + 1}.bias") for c in range(lay.nconv)]
        # split path: every conv's forward and dgrad weight images (and the
        # localiser's W2^T for the fused dense tail) in one launch per step
        # (paig_conv_wprep); the interpreter takes them per conv
        wp = {}
        wpf = wpd = None
        if cm == self.CONV_MATH["split"]:
            flags |= 8
            jobs = []
            for c, W_ in enumerate(Ws):
                cout, cin, ks = W_.shape[0], W_.shape[1], W_.shape[-1]
                jobs.append((c, 0, W_, cin, cout, ks))
                if c > 0:   # the dgrad kernel's images (Q10: none for the input layer)
                    jobs.append((c, 1, W_, cout, cin, ks))
            sizes = [int(L.paig_conv_wprep_size(j[3], j[4], j[5])) for j in jobs]
            if self.dense_tail(sw):
                jobs.append((-1, 2, self.p("encoder.l2.weight"), 200, 200, 1))
                sizes.append(2 * 200 * 200)
            buf = torch.empty(sum(-(-n // 8) * 8 for n in sizes), dtype=torch.int16, device=dev)
            outs, off = [], 0
            for j, n in zip(jobs, sizes):
                wp[(j[0], j[1])] = buf.data_ptr() + 2 * off
                outs.append(wp[(j[0], j[1])])
                off += -(-n // 8) * 8   # 16-byte aligned images
            n = len(jobs)
            # deferred: the U-Net's first conv carries the prep in its own
            # launch (PAIG_WPREP_MERGE=0: a separate launch, the A/B)
            wprep = L.paig_conv_wprep_defer if sw.wprep_merge else L.paig_conv_wprep
            wprep(n, (ctypes.c_void_p * n)(*[ptr(j[2]) for j in jobs]),
                  (ctypes.c_int * n)(*[j[3] for j in jobs]), (ctypes.c_int * n)(*[j[4] for j in jobs]),
                  (ctypes.c_int * n)(*[j[5] for j in jobs]), (ctypes.c_int * n)(*[j[1] for j in jobs]),
                  (ctypes.c_void_p * n)(*outs), st)
            S.wprep_buf = buf
            wpf = _parr([wp[(c, 0)] for c in range(lay.nconv)])
            wpd = _parr([wp.get((c, 1), 0) for c in range(lay.nconv)])
        S.wprep = wp
        nb = int(L.paig_unet_workspace_ex(lay.net, F, H, K, cm, flags))
        if nb <= 0:
            raise PaigError(f"paig_unet_workspace_ex: no U-Net for net={lay.net} F={F} H={H} K={K} math={cm}")
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        logits = None if fuse_head else _empty(F * K * lay.HW, dev)
        probe = self._unet_probe(S)
        L.paig_unet_fwd_ex(lay.net, F, H, K, cm, flags, *S.x_view, _parr([ptr(t) for t in Ws]),
                           _parr([ptr(t) for t in Bs]), ptr(logits), wpf, wpd, ptr(ws), nb, probe, None, st)
        if fuse_head:
            off = int(L.paig_unet_buffer(lay.net, F, H, K, cm, flags, 0, lay.head_buf))
            S.head_in = ws[off:off + F * lay.head_ci * lay.HW * 4].view(torch.float32)
        S.logits, S.unet_ws, S.unet_flags, S.unet_wp = logits, ws, flags, (wpf, wpd)

    def _unet_grad(self, S, buf, n):
        """The U-Net workspace's gradient buffer `buf` (n floats)."""
        lay = S.lay
        off = int(self.L.paig_unet_buffer(lay.net, lay.F, lay.H, lay.K, S.cm, S.unet_flags, 1, buf))
        assert off >= 0, f"no gradient buffer {buf} in the U-Net workspace"
        return S.unet_ws[off:off + n * 4].view(torch.float32)

    def _encoder_forward(self, S, st):
        """ConvolutionalEncoder.forward (nn/network/blocks.py:77-103) over the
        frames of S.x_view: U-Net, mask softmax x image, l1/l2, position head."""
        L = self.L
        lay, x_view, ws, dev = S.lay, S.x_view, S.ws, S.dev
        F, H, HW, K = lay.F, lay.H, lay.HW, lay.K
        self._unet_forward(S, st, fuse_head=lay.fuse_head)
        # ---- mask softmax + masked objects + localiser MLP + position head
        masks = _empty(F * (K + 1) * HW, dev)
        objs = _empty(K * F * 3 * HW, dev)
        pobjs = _empty(K * F * lay.l1_in, dev) if lay.unet else None
        if lay.fuse_head:   # the head conv + cat(ones) + softmax + mask x image (+ AvgPool2d), one launch
            hn = lay.prefix + lay.head_name
            L.paig_head_mask_fwd_ex(ptr(S.head_in), ptr(self.p(hn + ".weight")), ptr(self.p(hn + ".bias")),
                                    *x_view, ptr(masks), ptr(objs), ptr(pobjs), F, K, lay.head_ci, H, H,
                                    lay.head_flags, st)
        else:
            L.paig_mask_softmax_fwd(ptr(S.logits), *x_view, ptr(masks), ptr(objs), ptr(pobjs), F, K, 3, H, H, st)
        l1_x = pobjs if lay.unet else objs
        h1 = _empty(K * F * 200, dev)
        h2 = _empty(K * F * 200, dev)
        h3 = _empty(K * F * 2, dev)
        if not self.dense_tail(S.sw):
            self.linear(l1_x, K * F, "encoder.l1", h1, 1, st, ws)
            self.linear(h1, K * F, "encoder.l2", h2, 1, st, ws)
            enc_pos = _empty(F * 2 * K, dev)
            L.paig_head_fwd(ptr(h2), ptr(self.p("encoder.l3.weight")), ptr(self.p("encoder.l3.bias")), ptr(h3),
                            ptr(enc_pos), F, K, 200, float(H / 2), st)
        else:
            # l1 (blocks.py:98) as split-K slabs, then ONE launch for its
            # epilogue, l2 and the position head (blocks.py:99-102)
            S.dense_tail = True
            n1, KF = lay.l1_in, K * F
            enc_pos = _empty(F * 2 * K, dev)
            with self._p("gemm_fwd:encoder.l1", 2 * KF * 200 * n1, 4 * (KF * n1 + 200 * n1)):
                nS = L.paig_gemm_parts(0, 1, KF, 200, n1, ptr(l1_x), n1, ptr(self.p("encoder.l1.weight")), n1, ptr(ws),
                                       ws.numel(), self.gemm_math(self.FWD), st)
            if nS <= 0:
                raise PaigError(f"paig_gemm_parts failed (rc={nS}): {L.paig_last_error().decode(errors='replace')}")
            with self._p("dense_tail_fwd", 2 * KF * 200 * 200 + 4 * KF * 200,
                         4 * (nS * KF * 200 + 2 * KF * 200 + 200 * 200 + 2 * KF + 2 * KF)):
                w2t = S.wprep.get((-1, 2))   # W2^T from the step's weight-prep launch
                w2 = None if w2t is not None else self.p("encoder.l2.weight")
                if w2t is None:
                    S.w2t = _empty(200 * 200, dev)
                    w2t = ptr(S.w2t)
                L.paig_dense_tail_fwd(ptr(ws), nS, ptr(self.p("encoder.l1.bias")), ptr(h1), ptr(w2), w2t,
                                      ptr(self.p("encoder.l2.bias")), ptr(h2),
                                      ptr(self.p("encoder.l3.weight")), ptr(self.p("encoder.l3.bias")), ptr(h3),
                                      ptr(enc_pos), F, K, 200, float(H / 2), st)
        S.masks, S.objs, S.l1_x, S.h1, S.h2, S.h3, S.enc_pos = masks, objs, l1_x, h1, h2, h3, enc_pos

    # -- backward --------------------------------------------------------
    def backward(self, S, d_sse_rec=None, d_sse_roll=None, d_out=None, d_recons=None, d_enc_pos=None, d_pvs=None,
                 roll_live=0, lossw=None):
        """Writes every live parameter gradient into the model's flat grad buffer.
        roll_live > 0: only the first roll_live rollout steps of every
        sequence have a loss weight (the others' d_sse_roll entries are zero
        and there is no dense d_out): the rollout decoder backward reads only
        those frames.  lossw: {"rec" / "roll": (mode, LossAdjoints)} -- that
        decoder forms its per-frame weights in-kernel from the loss adjoints
        (paig_decoder_bwd_ex) instead of reading d_sse_*."""
        S.check_fresh()
        lay, sw, dev, L = S.lay, S.sw, S.dev, self.L
        st = stream_handle(dev)
        K, F, H, h, D, B, R = lay.K, lay.F, lay.H, lay.h, lay.D, lay.B, lay.R
        lossw = dict(lossw or {})

        if (K, H) not in ((2, 32), (3, 36), (2, 64)):
            # in-kernel weights need the one-CU decoders: materialise them here
            if "rec" in lossw:
                d_sse_rec = materialise(lossw.pop("rec")[1], 1, dev)
            if "roll" in lossw:
                d_sse_roll = materialise(lossw.pop("roll")[1], 2, dev)
        if d_out is not None:
            d_out = d_out.contiguous()
        if d_recons is not None:
            d_recons = d_recons.contiguous()

        # ---- buffers of the whole decoder / rollout / velocity backward
        dec = self._decoder_ops(S)
        slab_len = dec.slab_len
        roll_live = roll_live if (d_out is None and 0 < roll_live < R) else 0
        learn = S.sigma.has_grad
        dsig_rec = dsig_roll = None
        if learn:   # every frame's dL/dsigma, both decoders' arrays
            dsig = _empty(F + B * R, dev, torch.float64)
            dsig_rec, dsig_roll = ptr(dsig), ptr(dsig) + F * 8
        (nb_rec, scr_rec), (nb_roll, scr_roll) = dec.bwd_sizes(F), dec.bwd_sizes(B * R, R, roll_live)
        slab = _empty((nb_rec + nb_roll) * slab_len, dev)
        scratch = _empty(max(scr_rec, scr_roll), dev) if max(scr_rec, scr_roll) else None
        denc = _empty(F * D, dev)   # d enc_pos [B][Te][D]
        dpos_roll = _empty(B * R * D, dev)
        dsrc = _empty(slab_len, dev)
        dpos0 = _empty(B * D, dev)
        dvel0 = _empty(K * B * 2, dev) if S.vel0 is not None else None
        rops = self._rollout_ops(lay)
        rpart = _empty(rops.part_doubles(), dev, torch.float64)
        dXv = vslab = None
        if S.vel0 is not None:
            dXv = _empty(K * B * 2 * (lay.ins - 1 if lay.alt_vel else lay.ins), dev)
            if not lay.alt_vel:
                vblk, vlen = L.paig_velmlp_bwd_blocks(K * B), L.paig_velmlp_slab_len(lay.ins)
                vslab = _empty(vblk * vlen, dev)
        vparts = [_empty(L.paig_vfn_bwd_blocks(P) * 200, dev) for P in lay.vfn_sizes]
        if d_pvs is not None:
            d_pvs = d_pvs.contiguous()
        if d_enc_pos is not None:
            d_enc_pos = d_enc_pos.contiguous()

        # ---- rollout-frame decoder backward: d rollout positions + partial source grads
        live_frames = B * roll_live if roll_live else B * R
        with self._p("dec_bwd:rollout", 0,
                     self._dec_bwd_bytes(live_frames, B * R, lay, d_out is not None, S.tgt_roll.value_bytes)):
            dec.bwd(self._roll_pos(S), S.tgt_roll, ptr(d_sse_roll), lossw.get("roll"), ptr(d_out), lay.frame,
                    ptr(dpos_roll), ptr(slab) + nb_rec * slab_len * 4, ptr(scratch), B * R, roll_live, st, dsig_roll)

        # ---- rollout adjoint -> d pos0, d vel0, physics params; velocity encoder backward
        if rops.learned and S.roll_ws is None:
            raise PaigError(f"{self.model.cell_type}: the forward saved no workspace for its backward")
        with self._p(lay.spec.family.probe_bwd):
            rops.bwd(ptr(S.pvs), ptr(dpos_roll), ptr(d_pvs), ptr(dpos0), ptr(dvel0),
                     [ptr(self.g("rollout_cell." + n)) for n in lay.spec.names], ptr(rpart), S.roll_ws, 0, st)
        if S.vel0 is not None and lay.alt_vel:
            self.linear_bwd(S.Xv, dvel0, K * B, "velocity_encoder.init_vel_linear", dXv, None, 0, st, S.ws)
        elif S.vel0 is not None:   # one launch; its partial weight grads join the U-Net's batched slab reduction
            W0, _, W2, _, W4, _ = self._velmlp_params()
            L.paig_velmlp_bwd(ptr(dvel0), ptr(S.Xv), ptr(S.v1), ptr(S.v2), W0, W2, W4, ptr(dXv), ptr(vslab), K * B,
                              lay.ins, st)
            pm = "velocity_encoder.init_vel_mlp."
            g0 = self.g(pm + "0.weight")
            assert self.g(pm + "4.bias").data_ptr() == g0.data_ptr() + (vlen - 2) * 4, \
                "velocity MLP grads not contiguous"
            S.extra_slabs.append((vslab, vblk, vlen, g0))

        # ---- reconstruction decoder backward: d enc_pos + partial source grads
        with self._p("dec_bwd:recon", 0, self._dec_bwd_bytes(F, F, lay, d_recons is not None)):
            dec.bwd((ptr(S.enc_pos), 0, 2 * K, 0), S.tgt_rec, ptr(d_sse_rec), lossw.get("rec"), ptr(d_recons), lay.frame,
                    ptr(denc), ptr(slab), ptr(scratch), F, 0, st, dsig_rec)
        if learn:   # both decoders' dL/dsigma -> d loss / du (chain rule), into u's flat gradient slot
            L.paig_sigma_grad(dsig_rec, F, dsig_roll, B * R, ptr(self.p("decoder_sigma_u")),
                              ptr(self.g("decoder_sigma_u")), 0, st)

        # ---- source-gradient reduction (both decoders' slab rows), then the VFN
        # backward: whole, or phase 1 here and phase 2 inside the head backward's launch
        L.paig_slab_reduce_multi(1, (ctypes.c_void_p * 1)(ptr(slab)), (ctypes.c_int * 1)(nb_rec + nb_roll),
                                 (ctypes.c_int * 1)(slab_len), (ctypes.c_void_p * 1)(ptr(dsrc)), 0, st)
        vfn2 = self._vfn_bwd_args(S, dsrc, vparts)
        if sw.fuse_vel and sw.fuse_vfn2:
            L.paig_vfn_bwd1_multi(*vfn2, st)
        else:
            L.paig_vfn_bwd_multi(*vfn2, st)
            vfn2 = None
        if d_enc_pos is not None:
            L.paig_axpby(ptr(d_enc_pos), ptr(denc), F * D, 1.0, 1.0, st)
        # the velocity encoder's input gradient (dXv, dpos0, B, Te, ins, alt) is
        # added inside the head backward (PAIG_FUSE_VEL=0: the separate
        # unpack-add launch)
        vel = (ptr(dXv), ptr(dpos0), B, lay.Te, lay.ins, int(lay.alt_vel))
        if not sw.fuse_vel:
            L.paig_vel_unpack_add(vel[0], vel[1], ptr(denc), B, lay.Te, K, lay.ins, int(lay.alt_vel), st)
            vel = None
        self._encoder_backward(S, denc, st, vel=vel, vfn2=vfn2)

    def _encoder_backward(self, S, denc, st, hook=True, vel=None, vfn2=None):
        """ConvolutionalEncoder backward from d enc_pos (denc [F][2K]): position
        head, l2/l1, mask softmax, U-Net; all its weight gradients.  vel: the
        velocity term (dXv, dpos0, B, Te, ins, alt) the head backward adds to
        denc first, or None; vfn2: the VFN backward's phase 2 arguments
        (_vfn_bwd_args) riding in the same launch, or None."""
        lay, dev, ws, x_view, L = S.lay, S.dev, S.ws, S.x_view, self.L
        K, F, HW, H = lay.K, lay.F, lay.HW, lay.H
        # ---- position head + localiser MLP backward -> d masked objects
        dh2 = _empty(K * F * 200, dev)
        dh1 = _empty(K * F * 200, dev)
        fused_l2 = S.dense_tail   # l2's data gradient formed inside the head backward's launch
        hblk = L.paig_head_l2_bwd_blocks(K * F) if fused_l2 else L.paig_head_bwd_blocks(K * F)
        hslab = _empty(hblk * (2 * 200 + 2), dev)
        head = self._head_bwd_prefix(S, denc, dh2, hslab)
        if fused_l2:
            L.paig_head_l2_bwd(*head, *(vel or _NO_VEL), ptr(self.p("encoder.l2.weight")), ptr(S.h1), ptr(dh1),
                               *(vfn2 or _NO_VFN2), st)
        elif vfn2 is not None:
            L.paig_head_bwd_vel_vfn2(*head, *vel, *vfn2, st)
        elif vel is not None:
            L.paig_head_bwd_vel(*head, *vel, st)
        else:
            L.paig_head_bwd(*head, st)
        g3 = self.g("encoder.l3.weight")
        assert self.g("encoder.l3.bias").data_ptr() == g3.data_ptr() + 400 * 4, "l3 grads not contiguous"
        S.extra_slabs.append((hslab, hblk, 402, g3))
        dobjs = _empty(K * F * lay.l1_in, dev)
        # l2's weight-gradient epilogue rides in l1's weight-gradient launch, and
        # l1's in l1's data-gradient launch (neither reads the deferred output;
        # l1's weight gradient takes the workspace past l2's partial slabs).
        # PAIG_GEMM_EPI_MERGE=0: separate epilogue launches (the A/B)
        merge = S.sw.gemm_epi_merge and not self.probe
        w2 = int(L.paig_gemm_workspace(200, 200, K * F)) if merge else 0
        self.linear_bwd(S.h1, dh2, K * F, "encoder.l2", dh1, S.h1, 1, st, ws, need_dx=not fused_l2,
                        defer_epi=merge)
        self.linear_bwd(S.l1_x, dh1, K * F, "encoder.l1", dobjs, None, 0, st, ws[w2:] if merge else ws,
                        defer_epi=merge)
        if merge:
            L.paig_gemm_flush(st)
        # every gradient of the flat buffer's early bucket is final (queued on
        # this stream): the data-parallel all-reduce of that bucket may start
        if hook and self.bucket_hook is not None:
            self.bucket_hook()

        # ---- mask softmax backward (incl. ReLU' of ShallowUNet's c13, Q13, and
        # the AvgPool2d backward of the UNet path)
        if S.head_in is not None:
            # fused head + softmax backward: the head input's dY (its
            # producer's ReLU' applied), written straight into the U-Net
            # workspace's gradient buffer, and the head's weight/bias partials
            # (one slab row per block)
            hn, c = lay.prefix + lay.head_name, lay.head_ci
            dXl = self._unet_grad(S, lay.head_buf, F * c * HW)
            nb = L.paig_head_mask_blocks(F, H, H)
            nw = K * c + K
            hs = _empty(nb * nw, dev)
            L.paig_head_mask_bwd_ex(ptr(S.head_in), ptr(self.p(hn + ".weight")), ptr(self.p(hn + ".bias")),
                                    *x_view, ptr(S.masks), ptr(dobjs), ptr(dXl), ptr(hs), F, K, c, H, H,
                                    lay.head_flags, st)
            gh = self.g(hn + ".weight")
            assert self.g(hn + ".bias").data_ptr() == gh.data_ptr() + K * c * 4, "head grads not contiguous"
            S.extra_slabs.append((hs, nb, nw, gh))
            self._unet_backward(S, None, st)
        else:
            dLG = _empty(F * K * HW, dev)
            L.paig_mask_softmax_bwd(ptr(S.logits), *x_view, ptr(S.masks), ptr(dobjs), ptr(dLG), F, K, 3, H, H,
                                    (1 if lay.lg_relu else 0) | (2 if lay.unet else 0), st)
            self._unet_backward(S, dLG, st)

    def _unet_backward(self, S, dlogits, st):
        """The U-Net backward (paig_unet_bwd_ex, the same C interpreter as the
        forward) from d logits, or (fused head) from the head input's
        gradient already in the workspace; every conv's weight and bias
        gradient, with the step's other partial-gradient slabs (extra_slabs:
        head, l3, velocity MLP) in one batched deterministic reduction."""
        S.check_fresh()
        lay = S.lay
        L = self.L
        Ws = [self.p(lay.prefix + f"c{c + 1}.weight") for c in range(lay.nconv)]
        dwb = []
        for c in range(lay.nconv):
            gw = self.g(lay.prefix + f"c{c + 1}.weight")
            assert self.g(lay.prefix + f"c{c + 1}.bias").data_ptr() == gw.data_ptr() + gw.numel() * 4, \
                "flat grads: weight and bias must be adjacent"
            dwb.append(ptr(gw))
        extra = S.extra_slabs
        n = len(extra)
        ws = S.unet_ws
        _, wpd = S.unet_wp
        L.paig_unet_bwd_ex(lay.net, lay.F, lay.H, lay.K, S.cm, S.unet_flags, *S.x_view,
                           _parr([ptr(t) for t in Ws]), ptr(S.logits), ptr(dlogits), _parr(dwb), n,
                           _parr([ptr(e[0]) for e in extra]), _iarr([e[1] for e in extra]),
                           _iarr([e[2] for e in extra]), _parr([ptr(e[3]) for e in extra]), wpd, ptr(ws), ws.numel(),
                           self._unet_probe(S), None, st)
        S.release()
