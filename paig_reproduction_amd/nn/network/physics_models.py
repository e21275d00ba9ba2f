"""PhysicsNet — the reference's model surface (nn/network/physics_models.py:40-330)
on the MI355X-native step.

Same constructor signature/positional order, attributes, state_dict keys and
init RNG stream as the reference, so it is a drop-in for
runners/torch_run_physics.py.  ``forward``/``conv_feedforward`` run the whole
step (encoder U-Net -> localiser -> velocity MLP -> physics rollout -> STN
decoder, fused per-frame SSE) through libpaig_hip.so as ONE autograd node whose
backward is the explicit HIP backward (paig_reproduction_amd.engine).
"""
import inspect
import logging
import os
import weakref

import ctypes

import numpy as np
import torch
import torch.nn as pnn

from paig_reproduction_amd._lib import lib, ptr, stream_handle, require_device
from paig_reproduction_amd.engine import Engine, LossAdjoints, live_steps, materialise
from paig_reproduction_amd.flat import FlatParams
from paig_reproduction_amd.rollout_ops import SPECS
from paig_reproduction_amd.nn.network.base import OPTIMIZERS, BaseNetTorch
from paig_reproduction_amd.nn.network.blocks import ConvolutionalEncoder, VelocityEncoder, VariableFromNetwork
from paig_reproduction_amd.nn.network.cells import (bouncing_ode_cell, spring_ode_cell, gravity_ode_cell,
                                                    spring2d_ode_cell, bouncing2d_ode_cell, lstm_ode_cell,
                                                    interaction_ode_cell)

logger = logging.getLogger("tf")

CELLS = {
    "bouncing_ode_cell": bouncing_ode_cell,
    "spring_ode_cell": spring_ode_cell,
    "gravity_ode_cell": gravity_ode_cell,
    # opt-in (--physics_2d): the spring / bouncing cells with split size 2
    "spring2d_ode_cell": spring2d_ode_cell,
    "bouncing2d_ode_cell": bouncing2d_ode_cell,
    # opt-in (--blackbox_dynamics): a learned LSTM step in the place of the equations
    "lstm_ode_cell": lstm_ode_cell,
    # opt-in (--interaction_dynamics): a learned interaction network in the place of the equations
    "interaction_ode_cell": interaction_ode_cell,
    "lstm": pnn.LSTMCell,
}

COORD_UNITS = {
    "bouncing_balls": 8,
    "spring_color": 8,
    "spring_color_half": 8,
    "3bp_color": 12,
    "mnist_spring_color": 8,
}


class _LossHandoff:
    """What the _LossReduce backwards of ONE forward leave for that forward's
    _PhysicsStep.backward: per SSE output (reconstruction / rollout frames) a
    list of (in_kernel, LossAdjoints), one entry per compute_loss() whose
    loss reached the backward.  It lives on the forward's
    autograd context, so another model, another forward or an earlier backward
    can neither overwrite nor outlive it."""
    __slots__ = ("rec", "roll")

    def __init__(self):
        self.rec, self.roll = [], []

    def take(self):
        out = (self.rec[:], self.roll[:])
        del self.rec[:], self.roll[:]
        return out


def _materialise_lossw(entries, mode, dev):
    """The per-frame weights of in-kernel hand-off entries as an array (the
    rare paths: several losses on one forward, or a user gradient on the
    public SSE as well): one paig_loss_bwd per entry, summed."""
    w = None
    for _, adj in entries:
        wi = materialise(adj, mode, dev)
        w = wi if w is None else w + wi
    return w


class _PhysicsStep(torch.autograd.Function):
    """The whole forward as one node; backward = engine.backward.

    The per-frame SSE leaves it twice: sse_rec / sse_roll are the public
    tensors (PhysicsNet._sse_rec / _sse_roll; a gradient arriving there is an
    ordinary array of values), priv_rec / priv_roll alias the same memory and
    are consumed by compute_loss alone.  Only _LossReduce.backward ever
    returns a gradient for the private pair, and it says what that gradient
    means through the forward's _LossHandoff, so a NaN stand-in never meets a
    user gradient."""

    @staticmethod
    def forward(ctx, anchor, x, engine, grad_mode=True):
        # grad_mode: the caller's grad mode (inside a Function's forward it is
        # always off); under no_grad no backward can follow, and the
        # interaction cell then saves no activations
        need = ctx.needs_input_grad[0]
        res, S = engine.forward(x, need_saved=need, grad_mode=grad_mode)
        ctx.engine = engine
        ctx.S = S
        ctx.hand = engine.last_loss_handoff = _LossHandoff()
        ctx.set_materialize_grads(False)
        engine.last_masked_objs = res["masked_objs"]
        outs = (res["output_seq"], res["recons_out"], res["enc_pos"], res["pos_vel_seq"], res["sse_rec"],
                res["sse_roll"], res["sse_rec"].detach(), res["sse_roll"].detach(), res["enc_masks"], res["template"],
                res["contents"], res["background_content"])
        ctx.mark_non_differentiable(res["enc_masks"], res["template"], res["contents"], res["background_content"])
        return outs

    @staticmethod
    def _weights(pub, priv, entries, mode):
        """One SSE output's incoming gradients -> (weight array or None,
        in-kernel loss weights (mode, adjoints) or None)."""
        if not entries:
            return pub, None
        kinds = {e[0] for e in entries}
        if len(kinds) > 1:
            raise RuntimeError("PhysicsNet: loss-weight modes mixed within one backward")
        if kinds == {True}:
            if len(entries) == 1 and pub is None:
                return None, (mode, entries[0][1])
            # the private gradient is a (sum of) NaN stand-ins: form the values
            w = _materialise_lossw(entries, mode, priv.device)
        else:
            w = priv   # the weight arrays themselves, summed by autograd
        return (w if pub is None else w + pub), None

    @staticmethod
    def backward(ctx, d_out, d_rec, d_enc, d_pvs, d_sse_rec, d_sse_roll, d_priv_rec, d_priv_roll, *unused):
        if ctx.S is None:
            raise RuntimeError("PhysicsNet step was run without saving activations")
        ent_rec, ent_roll = ctx.hand.take()
        flat = ctx.engine.model._flat
        acc = flat.begin_backward()
        # decided afresh in every backward from what reached THIS forward
        live = live_steps(d_out, d_sse_roll, ent_roll)
        w_rec, lw_rec = _PhysicsStep._weights(d_sse_rec, d_priv_rec, ent_rec, 1)
        w_roll, lw_roll = _PhysicsStep._weights(d_sse_roll, d_priv_roll, ent_roll, 2)
        # incoming gradients may be broadcast views (d sum(sse)/d sse is an
        # expanded scalar, stride 0): the kernels read dense vectors
        w_rec = w_rec.contiguous() if w_rec is not None else None
        w_roll = w_roll.contiguous() if w_roll is not None else None
        lw = {k: v for k, v in (("rec", lw_rec), ("roll", lw_roll)) if v is not None}
        ctx.engine.backward(ctx.S, w_rec, w_roll, d_out, d_rec, d_enc, d_pvs, roll_live=live, lossw=lw)
        # nothing reached the rollout branch (quirk Q1: the loss read a stale
        # output): the velocity encoder and physics parameters are not in the
        # graph, so like torch they get grad None (their flat slots hold zeros)
        no_roll = d_out is None and w_roll is None and lw_roll is None and d_pvs is None
        flat.end_backward(acc, ctx.engine.model.ROLLOUT_PARAMS if no_roll else ())
        ctx.S = None
        return None, None, None, None


_LOSSW = {}


def _lossw_buffers(dev, n_rec, n_roll):
    """Persistent NaN-filled stand-ins for the loss-weight gradients (one pair
    per device and size; filled once, outside any graph capture: the first
    training steps run eagerly).  They carry nothing: whoever reads one as
    values gets NaN, never silent garbage."""
    key = (str(dev), n_rec, n_roll)
    if key not in _LOSSW:
        _LOSSW[key] = (torch.full((n_rec,), float("nan"), device=dev), torch.full((n_roll,), float("nan"), device=dev))
    return _LOSSW[key]


class _LossReduce(torch.autograd.Function):
    """Per-frame SSE -> (train, extrap, recons) (physics_models.py:119-141):
    train = pred + ae * recons formed in the kernel -- the value the
    reference's in-place ``+=`` leaves in BOTH train_loss and pred_loss (Q2)."""

    @staticmethod
    def forward(ctx, sse_rec, sse_roll, B, Te, R, pred, ae, hand_rec, hand_roll):
        """hand_rec / hand_roll: the _LossHandoff lists of the forward whose
        PRIVATE SSE output sse_rec / sse_roll is, or None for any other
        tensor (its gradient is then always an array of values)."""
        dev = sse_rec.device
        o = [torch.empty((), device=dev) for _ in range(3)]
        lib().paig_loss_reduce(ptr(sse_rec), ptr(sse_roll), B, Te, R, pred, float(ae), ptr(o[0]), ptr(o[1]),
                               ptr(o[2]), stream_handle(dev))
        ctx.shape = (B, Te, R, pred, float(ae))
        ctx.dev = dev
        ctx.hands = (hand_rec, hand_roll)
        ctx.set_materialize_grads(False)
        return o[0], o[1], o[2]

    @staticmethod
    def backward(ctx, dt, de, dr):
        B, Te, R, pred, ae = ctx.shape
        lw = LossAdjoints(dt, de, dr, ae, B, Te, R, pred)
        # in-kernel: the per-frame weights are formed inside the decoder
        # backwards from these adjoints (paig_decoder_bwd_ex lw modes).  The
        # adjoints travel on the forward's hand-off; the returned gradient is
        # a persistent NaN buffer that only tells autograd the path is live.
        inkernel = os.environ.get("PAIG_LOSSW_INKERNEL", "1") != "0" and not torch.is_grad_enabled()
        standin = _lossw_buffers(ctx.dev, B * Te, B * R)
        grads, arrays = [None, None], [None, None]
        for i, hand in enumerate(ctx.hands):
            if not ctx.needs_input_grad[i]:
                continue
            if i == 1 and dt is None and de is None:
                continue   # only the reconstruction loss is in the graph: the rollout SSE gets no gradient
            if hand is not None:
                hand.append((inkernel, lw))
            if hand is not None and inkernel:
                grads[i] = standin[i]
            else:
                grads[i] = arrays[i] = torch.empty(B * (R if i else Te), device=ctx.dev)
        if arrays[0] is not None or arrays[1] is not None:
            lib().paig_loss_bwd(ptr(dt), ptr(de), ptr(dr), ae, ptr(arrays[0]), ptr(arrays[1]), B, Te, R, pred,
                                stream_handle(ctx.dev))
        return grads[0], grads[1], None, None, None, None, None, None, None


class _FrameSSE(torch.autograd.Function):
    """Per-frame SSE of dense frames vs input[:, ins:] (the unfused path, for a
    loss on frames that are not the current forward's, e.g. quirk Q1)."""

    @staticmethod
    def forward(ctx, frames, x, ins):
        B, R = frames.shape[0], frames.shape[1]
        T = x.shape[1]
        if x.shape[0] != B or tuple(x.shape[2:]) != tuple(frames.shape[2:]) or T - ins != R:
            # the reference's (input[:, ins:] - output) would not broadcast either
            raise RuntimeError(f"compute_loss: output {tuple(frames.shape)} does not match input[:, {ins}:] of "
                               f"{tuple(x.shape)}")
        fr = 3 * frames.shape[-1] * frames.shape[-2]
        frames = frames.contiguous()
        x = x.contiguous()
        sse = torch.empty(B * R, device=frames.device)
        lib().paig_frame_sse(ptr(frames), fr, 0, 0, ptr(x) + ins * fr * 4, T * fr, R, fr, ptr(sse), B * R, fr,
                             stream_handle(frames.device))
        ctx.save_for_backward(frames, x)
        ctx.meta = (ins, B, R, T, fr)
        return sse

    @staticmethod
    def backward(ctx, w):
        frames, x = ctx.saved_tensors
        ins, B, R, T, fr = ctx.meta
        d = torch.empty_like(frames)
        lib().paig_frame_sse_bwd(ptr(frames), fr, 0, 0, ptr(x) + ins * fr * 4, T * fr, R, fr, ptr(w.contiguous()),
                                 ptr(d), B * R, fr, stream_handle(frames.device))
        return d, None, None


class PhysicsNet(BaseNetTorch):
    def __init__(self,
                 task="",
                 recurrent_units=128,
                 lstm_layers=1,
                 cell_type="",
                 seq_len=20,
                 input_steps=3,
                 pred_steps=5,
                 autoencoder_loss=0.0,
                 alt_vel=False,
                 color=False,
                 input_size=36 * 36,
                 encoder_type="",
                 decoder_type="conv_st_decoder",
                 device=torch.device("cpu"),
                 sigma=1.0,
                 learn_sigma=False):
        super().__init__()
        self.learn_sigma = False
        self.device = device
        assert task in COORD_UNITS
        self.task = task
        self.recurrent_units = recurrent_units
        self.lstm_layers = lstm_layers
        self.cell_type = cell_type
        self.cell = CELLS[self.cell_type]
        if self.cell is pnn.LSTMCell:
            raise NotImplementedError("the 'lstm' black-box cell cannot be called by the reference's rollout "
                                      "(physics_models.py:233 signature mismatch); not supported: the black-box "
                                      "cell that rolls out is cell_type='lstm_ode_cell'")
        if self.cell is lstm_ode_cell and lstm_layers != 1:
            raise ValueError(f"lstm_ode_cell: lstm_layers={lstm_layers!r}, only 1 is supported")
        self.color = color
        self.conv_ch = 3 if color else 1
        if not color:
            # Q11: the template is tiled to 3 channels regardless of --color, so
            # grayscale breaks in the reference too.
            raise ValueError("PhysicsNet requires color=True (reference quirk Q11: grayscale is broken)")
        self.input_size = input_size
        self.conv_input_shape = [self.conv_ch] + [int(np.sqrt(input_size))] * 2
        self.input_shape = [self.conv_ch] + [int(np.sqrt(input_size))] * 2
        self.decoder = {name: method for name, method in
                        inspect.getmembers(self, predicate=inspect.ismethod) if "decoder" in name}[decoder_type]
        self.output_shape = self.conv_input_shape
        assert seq_len > input_steps + pred_steps
        assert input_steps >= 1
        assert pred_steps >= 1
        self.seq_len = seq_len
        self.input_steps = input_steps
        self.pred_steps = pred_steps
        self.extrap_steps = self.seq_len - self.input_steps - self.pred_steps
        self.alt_vel = alt_vel
        self.autoencoder_loss = autoencoder_loss
        self.coord_units = COORD_UNITS[self.task]
        self.n_objs = self.coord_units // 4
        self.extra_valid_fns.append((self.visualize_sequence, [], {}))
        self.extra_test_fns.append((self.visualize_sequence, [], {}))
        tmpl_size = self.conv_input_shape[1] // 2
        # physics_models.py:155-161: "This parameter can be played with" -- a
        # plain attribute (no parameter, not in the state_dict), read at every
        # forward (decoder_sigma)
        self.log_sig = sigma
        if learn_sigma:
            # the reference's original trainable logsigma (physics_models.py:
            # 155-161, kept there as a comment): sigma = exp(ln 2 tanh(u)) from
            # one fp32 parameter u, strictly inside SIGMA_RANGE for every u
            lo, hi = self.SIGMA_RANGE
            if not lo < float(sigma) < hi:
                raise ValueError(f"sigma={sigma!r}: a learnable sigma starts strictly inside ({lo}, {hi})")
            u0 = np.arctanh(np.log(np.float64(sigma)) / np.log(2.0))
        # Network subcomponents (creation order = reference order, for init parity)
        self.var_net_content = VariableFromNetwork([self.n_objs, self.conv_ch, tmpl_size, tmpl_size])
        self.var_net_background = VariableFromNetwork([1, *self.input_shape])
        self.var_net_template = VariableFromNetwork([self.n_objs, 1, tmpl_size, tmpl_size])
        self.encoder = ConvolutionalEncoder(self.conv_input_shape, 200, 2, self.n_objs, self.device)
        self.velocity_encoder = VelocityEncoder(self.alt_vel, self.input_steps, self.n_objs, self.coord_units,
                                                self.device)
        if SPECS[self.cell_type].units_ctor:
            self.rollout_cell = self.cell(self.coord_units // 2, self.coord_units // 2, recurrent_units,
                                          self.conv_input_shape[1] / 2)
        else:
            self.rollout_cell = self.cell(self.coord_units // 2, self.coord_units // 2)
        if learn_sigma:
            # fp32 on purpose: the base learning rate and the "decoder" group,
            # not the fp64 physics buffer's (flat.py)
            self.decoder_sigma_u = pnn.Parameter(torch.tensor(float(u0), dtype=torch.float32))
            self.learn_sigma = True
        object.__setattr__(self, "_sigma_dev", None)
        # the standalone U-Net / encoder forwards run on this model's engine
        for mod in (self.encoder, self.encoder.shallow_unet, self.encoder.unet):
            object.__setattr__(mod, "_paig_owner", weakref.ref(self))
        object.__setattr__(self, "_parts", None)
        self.loss_mode = "fresh"
        # conv arithmetic of the HIP path: "split" (fp32-accurate split-precision
        # 16-bit MFMA, default), "fp32" (f32-input MFMA) or "bf16"
        self.conv_math = os.environ.get("PAIG_CONV_MATH", "split")
        self._init_native()

    # ------------------------------------------------------------ native ----
    # gradients final before the U-Net backward starts (VariableFromNetwork and
    # the localiser's l1/l2: ~97% of the gradient bytes) lead the flat buffer,
    # so their data-parallel all-reduce can start while the U-Net backward runs
    EARLY_GRADS = ("var_net_content.", "var_net_background.", "var_net_template.", "encoder.l1.", "encoder.l2.")
    # parameters reached only through the rollout branch
    ROLLOUT_PARAMS = ("velocity_encoder.", "rollout_cell.")

    def _live_names(self):
        dead = "encoder.unet." if self.conv_input_shape[1] < 40 else "encoder.shallow_unet."
        names = []
        for n, p in self.named_parameters():
            if n.startswith(dead) or n.startswith("rollout_cell.") or n == "decoder_sigma_u":
                continue
            names.append(n)
        names = ([n for n in names if n.startswith(self.EARLY_GRADS)] +
                 [n for n in names if not n.startswith(self.EARLY_GRADS)])
        if self.learn_sigma:   # the last slot of the fp32 buffer's late part: every other offset as without it
            names.append("decoder_sigma_u")
        # the cell's trainable parameters last, in its kernels' gradient order (rollout_ops.SPECS)
        return names + ["rollout_cell." + n for n in SPECS[self.cell_type].names]

    def _init_native(self):
        object.__setattr__(self, "_flat", FlatParams(self, self._live_names(), early=self.EARLY_GRADS))
        object.__setattr__(self, "_engine", None)
        object.__setattr__(self, "_anchor", None)

    @property
    def _param_by_name(self):
        return dict(self.named_parameters())

    def _native(self):
        if self._engine is None:
            object.__setattr__(self, "_engine", Engine(self))
        self._flat.ensure()
        if self._anchor is None:
            object.__setattr__(self, "_anchor", torch.zeros((), requires_grad=True))
        return self._engine

    # ------------------------------------------------------------- API ----
    def get_batch(self, batch_size, iterator):
        batch_x, _ = iterator.next_batch(batch_size)
        feed_dict = {"input": batch_x}
        return feed_dict, (batch_x, None)

    def compute_loss(self):
        """nn/network/physics_models.py:119-142, including the in-place ``+=``
        that makes pred_loss alias train_loss (Q2)."""
        B, Te, R = self.input.shape[0], self.input_steps + self.pred_steps, self.pred_steps + self.extrap_steps
        # the forward's private SSE outputs and its loss hand-off (_PhysicsStep)
        sse_rec, (hand_rec, hand_roll) = self._sse_priv[0], self._sse_priv[2]
        if self.output is self._fwd_output:
            sse_roll = self._sse_priv[1]
        else:
            sse_roll, hand_roll = _FrameSSE.apply(self.output, self.input, self.input_steps), None
        # train = pred + ae * recons in one kernel; pred_loss IS train_loss, as
        # after the reference's in-place ``train_loss += ae * recons`` (Q2)
        train, extrap, recons = _LossReduce.apply(sse_rec, sse_roll, B, Te, R, self.pred_steps,
                                                  self.autoencoder_loss, hand_rec, hand_roll)
        self.recons_loss = recons
        self.pred_loss = train
        self.extrap_loss = extrap
        train_loss = self.pred_loss
        eval_losses = [self.pred_loss, self.extrap_loss, self.recons_loss]
        return train_loss, eval_losses

    def build_optimizer(self, base_lr, optimizer="rmsprop", anneal_lr=True, max_grad_norm=None, physics_lr_mult=None,
                        grad_norms=None):
        """The reference's positional signature (physics_models.py:144-149),
        plus the flat optimizer's gradient-norm options (FlatOptimizer); None
        falls back to the environment (PAIG_MAX_GRAD_NORM, PAIG_PHYSICS_LR_MULT,
        PAIG_GRAD_NORMS), as conv_math does, and from there to off."""
        self.base_lr = base_lr
        self.anneal_lr = anneal_lr
        self.lr = base_lr
        self._flat.ensure()
        if max_grad_norm is None:
            max_grad_norm = float(os.environ.get("PAIG_MAX_GRAD_NORM", "0"))
        if physics_lr_mult is None:
            physics_lr_mult = float(os.environ.get("PAIG_PHYSICS_LR_MULT", "1"))
        if grad_norms is None:
            grad_norms = os.environ.get("PAIG_GRAD_NORMS", "0").strip().lower() not in ("", "0", "false", "no")
        self.optimizer = OPTIMIZERS[optimizer](self, self.lr, max_grad_norm=max_grad_norm,
                                               physics_lr_mult=physics_lr_mult, grad_norms=grad_norms)

    SIGMA_RANGE = (0.5, 2.0)

    def __setattr__(self, name, value):
        if name == "log_sig" and self.__dict__.get("learn_sigma"):
            raise AttributeError("log_sig is fixed in learnable mode: set the parameter decoder_sigma_u "
                                 "(sigma = exp(ln 2 tanh(u)))")
        super().__setattr__(name, value)

    def sigma_buffer(self):
        """Learnable mode: the one-double device buffer the decoders read
        sigma from (paig_sigma_from_u writes it at the start of every forward).
        Persistent, so a captured step keeps its address."""
        dev = self.decoder_sigma_u.device
        if self._sigma_dev is None or self._sigma_dev.device != dev:
            object.__setattr__(self, "_sigma_dev", torch.ones(1, device=dev, dtype=torch.float64))
        return self._sigma_dev

    def decoder_sigma(self):
        """The decoders' attention-window scale of this forward, as the
        reference forms it (physics_models.py:160): np.exp(np.log(log_sig)), a
        float64.  The HIP decoders serve [0.5, 2].

        Learnable mode: exp(ln 2 tanh(u)) of the current decoder_sigma_u, in
        fp64 as the device forms it.  One device read: it SYNCHRONISES, so
        call it at log steps only (the step itself never does)."""
        if self.learn_sigma:
            u = np.float64(np.float32(self.decoder_sigma_u.detach().item()))
            return float(np.exp(np.log(2.0) * np.tanh(u)))
        with np.errstate(all="ignore"):
            sigma = float(np.exp(np.log(np.float64(self.log_sig))))
        lo, hi = self.SIGMA_RANGE
        if not lo <= sigma <= hi:
            raise ValueError(f"log_sig={self.log_sig!r}: the decoders support sigma in [{lo}, {hi}]")
        return sigma

    def conv_st_decoder(self, inp):
        """Decode positions [N, coord_units/2] -> frames [N, C, H, W]
        (physics_models.py:151-199): the three VariableFromNetwork sources and
        the HIP STN/compositing decoder, differentiable w.r.t. the positions and
        the sources' parameters.  Sets template / contents / background_content
        like the reference; transf_contents / transf_masks are formed on request."""
        require_device(inp)
        from paig_reproduction_amd.nn.network.native_modules import _STDecoder
        self._native()
        out = _STDecoder.apply(inp, self._anchor_for_modules(), self)
        srcs = self._last_sources
        K, H = self.n_objs, self.conv_input_shape[1]
        h = H // 2
        self.template = srcs["tmpl"].view(K, 1, h, h)
        self.contents = srcs["cont"].view(K, 3, h, h)
        self.background_content = srcs["bg"].view(1, 3, H, H)
        object.__setattr__(self, "_parts", (inp.detach().float().contiguous(), 2 * K, srcs, self._last_decoder_sigma))
        return out

    def check_numerics(self):
        """Raise if a split-precision kernel flagged an operand outside f16's
        range since the last check.  The step's operands (activations,
        gradients, weights) are all scaled by powers of two from their own
        maxima and have no range limit; the flag remains for the fixed-scale
        fallbacks of the C ABI (a conv weight gradient called without the
        forward's xmax slots, GEMM math 1 / 5), which the step never takes.
        Synchronises the device: BaseNetTorch calls it at log steps only."""
        if self.conv_math != "split":
            return
        rc = lib().paig_f16_range_status(1)
        if rc != 0:
            raise FloatingPointError(
                "split-precision path: an operand beyond the f16 staging range of a fixed-scale fallback "
                "kernel; rerun with --conv_math fp32" if rc > 0 else f"paig_f16_range_status failed ({rc})")

    def _anchor_for_modules(self):
        return torch.zeros((), requires_grad=True)

    _VFN_SRCS = (("var_net_template", "tmpl", 0), ("var_net_content", "cont", 0), ("var_net_background", "bg", 1))

    def _decoder_sources(self, dev, st):
        """The decoder's step-constant sources (physics_models.py:163-171,
        185-186): raw template, raw contents, sigmoid(background)."""
        L = lib()
        K, H = self.n_objs, self.conv_input_shape[1]
        h = H // 2
        sizes = {"tmpl": K * h * h, "cont": K * 3 * h * h, "bg": 3 * H * H}
        pd = self._param_by_name
        srcs = {}
        for nm, key, post in self._VFN_SRCS:
            P = sizes[key]
            srcs[nm] = (torch.empty(200, device=dev), torch.empty(P, device=dev),
                        torch.empty(P, device=dev) if post else None, P)
        arr = lambda xs: (ctypes.c_void_p * 3)(*xs)   # noqa: E731
        L.paig_vfn_fwd_multi(3, *[arr([ptr(pd[nm + suf]) for nm, _, _ in self._VFN_SRCS])
                                  for suf in (".l1.weight", ".l1.bias", ".l2.weight", ".l2.bias")],
                             arr([ptr(srcs[nm][0]) for nm, _, _ in self._VFN_SRCS]),
                             arr([ptr(srcs[nm][1]) for nm, _, _ in self._VFN_SRCS]),
                             arr([ptr(srcs[nm][2]) for nm, _, _ in self._VFN_SRCS]),
                             (ctypes.c_int * 3)(*[srcs[nm][3] for nm, _, _ in self._VFN_SRCS]), st)
        out = {"tmpl": srcs["var_net_template"][1], "cont": srcs["var_net_content"][1],
               "bg": srcs["var_net_background"][2], "_vfn": srcs}
        object.__setattr__(self, "_last_sources", out)
        return out

    def _decoder_sources_backward(self, srcs, dsrc, st):
        """dsrc = [d template | d sigmoid(content) | d sigmoid(background)] (the
        decoder's source gradients) -> the three VariableFromNetworks' parameter
        gradients, deposited into the flat gradient buffer."""
        from paig_reproduction_amd.flat import deposit_grad
        L = lib()
        dev = dsrc.device
        v = srcs["_vfn"]
        pd = self._param_by_name
        offs, o = [], 0
        for nm, _, _ in self._VFN_SRCS:
            offs.append(o)
            o += v[nm][3]
        g = {nm: {suf: torch.empty_like(pd[nm + suf]) for suf in (".l1.weight", ".l1.bias", ".l2.weight", ".l2.bias")}
             for nm, _, _ in self._VFN_SRCS}
        parts = [torch.empty(L.paig_vfn_bwd_blocks(v[nm][3]) * 200, device=dev) for nm, _, _ in self._VFN_SRCS]
        arr = lambda xs: (ctypes.c_void_p * 3)(*xs)   # noqa: E731
        # content and background enter through a sigmoid (sig = 1)
        L.paig_vfn_bwd_multi(3, arr([ptr(dsrc) + 4 * off for off in offs]),
                             arr([ptr(v[nm][1]) for nm, _, _ in self._VFN_SRCS]), (ctypes.c_int * 3)(0, 1, 1),
                             arr([ptr(v[nm][0]) for nm, _, _ in self._VFN_SRCS]),
                             arr([ptr(pd[nm + ".l2.weight"]) for nm, _, _ in self._VFN_SRCS]),
                             *[arr([ptr(g[nm][suf]) for nm, _, _ in self._VFN_SRCS])
                               for suf in (".l1.weight", ".l1.bias", ".l2.weight", ".l2.bias")],
                             arr([ptr(pt) for pt in parts]), (ctypes.c_int * 3)(*[v[nm][3] for nm, _, _ in self._VFN_SRCS]),
                             st)
        for nm, _, _ in self._VFN_SRCS:
            for suf, t in g[nm].items():
                deposit_grad(pd[nm + suf], t)

    def _transf_parts(self):
        """(transf_contents, transf_masks) of the last decoder call
        (physics_models.py:186-196): K warped contents + the tiled background,
        and the K+1 compositing masks, each [N, 3, H, W] (detached)."""
        if self._parts is None:
            raise AttributeError("transf_contents / transf_masks: no decoder call yet")
        cached = getattr(self, "_parts_cache", None)
        if cached is not None and cached[0] is self._parts:
            return cached[1]
        pos, inner, srcs, sigma = self._parts
        K, H = self.n_objs, self.conv_input_shape[1]
        N = pos.shape[0]
        dev = pos.device
        cont = torch.empty(K + 1, N, 3, H, H, device=dev)
        masks = torch.empty(K + 1, N, 3, H, H, device=dev)
        from paig_reproduction_amd.nn.network.native_modules import decoder_ops
        decoder_ops(self, srcs, sigma).parts(ptr(pos), inner, ptr(cont), ptr(masks), N, stream_handle(dev))
        res = ([cont[k] for k in range(K + 1)], tuple(masks[k] for k in range(K + 1)))
        object.__setattr__(self, "_parts_cache", (self._parts, res))
        return res

    @property
    def transf_contents(self):
        return self._transf_parts()[0]

    @property
    def transf_masks(self):
        return self._transf_parts()[1]

    def forward(self, input):
        return self.conv_feedforward(input)

    def conv_feedforward(self, inp):
        """nn/network/physics_models.py:204-245 as one fused native step."""
        require_device(inp)
        eng = self._native()
        self.input = inp
        x = inp.detach()
        if x.dtype != torch.float32:
            x = x.float()
        outs = _PhysicsStep.apply(self._anchor, x, eng, torch.is_grad_enabled())
        (out, recons, enc_pos, pvs, sse_rec, sse_roll, priv_rec, priv_roll, masks, tmpl, cont, bg) = outs
        hand = eng.last_loss_handoff
        object.__setattr__(self, "_sse_priv", (priv_rec, priv_roll, (hand.rec, hand.roll)))
        self.recons_out = recons
        self.enc_pos = enc_pos
        self.pos_vel_seq = pvs
        self.enc_masks = masks
        self.masked_objs = eng.last_masked_objs
        self.template, self.contents, self.background_content = tmpl, cont, bg
        self._sse_rec, self._sse_roll = sse_rec, sse_roll
        # the reference's last decoder call decodes the last rollout step
        R, D = self.pred_steps + self.extrap_steps, self.coord_units // 2
        object.__setattr__(self, "_parts", (pvs.detach()[:, R, :D], (R + 1) * 2 * D,
                                            {"tmpl": tmpl.detach(), "cont": cont.detach(), "bg": bg.detach()},
                                            eng.last_sigma))
        self._fwd_output = out
        return out

    def visualize_sequence(self):
        """physics_models.py:247-330, reduced to what this image supports:
        example%d.jpg grids and extra_outputs.npz (the gif needs moviepy,
        absent here).  Off the hot path."""
        try:
            import matplotlib
            matplotlib.use("agg")
            import matplotlib.pyplot as plt
        except Exception:  # pragma: no cover
            return
        batch_size = min(self.batch_size, 4)
        feed_dict, (batch_x, _) = self.get_batch(batch_size, self.test_iterator)
        if torch.is_tensor(batch_x):   # device-resident dataset (F2)
            batch_x = batch_x.detach().cpu().numpy()
        if not hasattr(self, "output") or self.output is None:
            return
        output_seq = self.output.detach().cpu().numpy()[:batch_size]
        recons_seq = self.recons_out.detach().cpu().numpy()[:batch_size]
        n = min(batch_size, output_seq.shape[0], batch_x.shape[0])
        for i in range(n):
            seq = np.concatenate([batch_x[i, :self.input_steps], output_seq[i]], 0)
            rows = [seq, batch_x[i], np.concatenate([recons_seq[i], np.zeros(
                (self.extrap_steps,) + recons_seq.shape[2:], dtype=recons_seq.dtype)], 0)]
            grid = np.concatenate([np.concatenate(list(r.reshape(r.shape[0], *self.input_shape[1:],
                                                                 self.conv_ch)), 1) for r in rows], 0)
            fig, ax = plt.subplots(figsize=(grid.shape[1] // 32, grid.shape[0] // 32 + 1))
            ax.imshow(np.clip(grid, 0, 1), interpolation="nearest")
            ax.axis("off")
            fig.savefig(os.path.join(self.save_dir, "example%d.jpg" % i))
            plt.close(fig)
        np.savez_compressed(os.path.join(self.save_dir, "extra_outputs.npz"),
                            contents=self.contents.detach().cpu().numpy(),
                            templates=self.template.detach().cpu().numpy(),
                            background_content=self.background_content.detach().cpu().numpy(),
                            enc_masks=self.enc_masks.detach().cpu().numpy())
