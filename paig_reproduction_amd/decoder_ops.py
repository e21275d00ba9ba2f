"""The decoder's C-ABI calls, chosen and packed in one place.

The ABI exports one decoder entry point per (operation, sigma kind, target
form); every caller above it (the engine, the standalone decoder module, the
parts query, the benchmarks) goes through DecoderOps, which picks the export
and lays out its positional arguments.  Sigma and Targets name the two
operands whose form selects the export.

Pure Python: nothing here allocates, reads the environment or touches torch
beyond ptr(); every device operand is an address (int, or None for NULL).
"""
from typing import NamedTuple

from ._lib import PaigError, ptr


class Sigma:
    """The attention-window scale of one forward: a host float (in [0.5, 2]),
    or the model's one-double device tensor (the learnable scale, which the
    host never reads)."""
    __slots__ = ("value",)

    def __init__(self, value):
        self.value = float(value) if isinstance(value, (int, float)) else value

    @property
    def on_device(self):
        return not isinstance(self.value, float)

    @property
    def suffix(self):
        """Of the entry points that take this sigma."""
        return "_sigma_dev" if self.on_device else "_sigma"

    @property
    def arg(self):
        """Their trailing sigma argument: the float / the device pointer."""
        return ptr(self.value) if self.on_device else self.value

    @property
    def has_grad(self):
        """Whether the backward can produce dL/dsigma (a device sigma only)."""
        return self.on_device


class Targets(NamedTuple):
    """The frames a decoder compares against: fp32 frames (f32), the dataset's
    bytes behind a row index (u8, idx), or none.  Frame f is at
    (f // grp) * fs + (f % grp) * gs elements (grp 0: f * fs)."""
    f32: object
    u8: object
    idx: object
    fs: int
    grp: int
    gs: int

    @classmethod
    def frames(cls, p, fs, grp, gs):
        return cls(p, None, None, fs, grp, gs)

    @classmethod
    def dataset_bytes(cls, base, idx_ptr, fs, grp, gs):
        return cls(None, base, idx_ptr, fs, grp, gs)

    @classmethod
    def none(cls):
        return cls(None, None, None, 0, 0, 0)

    @property
    def kind(self):
        form = (self.f32 is not None, self.u8 is not None)
        if form == (False, True):
            return "u8"
        if self.idx is None and form != (True, True):
            return "f32" if form[0] else "none"
        raise PaigError(f"decoder targets: an fp32 and a byte pointer, or a row index without bytes: {tuple(self)}")

    @property
    def value_bytes(self):
        """Bytes read per target value."""
        return 1 if self.kind == "u8" else 4


class DecoderOps:
    """The decoder calls of one (K, h, H), one Sigma and one set of sources
    (template, content, background pointers) on the library L."""

    def __init__(self, L, K, h, H, sigma, sources):
        self.L, self.shape, self.sigma, self.sources = L, (K, h, H), sigma, tuple(sources)

    def _fn(self, name):
        return getattr(self.L, "paig_decoder_" + name + self.sigma.suffix)

    def fwd(self, pos_view, out, out_fs, targets, sse, F, st, roll=None):
        """Decode F frames at pos_view (pointer, outer, inner, group) into out,
        with their SSE against targets into sse.  roll: the rollout's
        arguments (RolloutOps.merged_args) to run it in the same launch."""
        kind = targets.kind
        if kind != "none" and sse is None:
            raise PaigError("decoder fwd: targets without an SSE output")
        if kind == "none" and sse is not None:
            raise PaigError("decoder fwd: an SSE output without targets")
        if kind == "u8":
            tgt = (targets.u8, targets.idx)
        else:
            tgt = (targets.f32,)
        dec = (*pos_view, *self.sources, out, out_fs, *tgt, targets.fs, targets.grp, targets.gs, sse, F, *self.shape,
               self.sigma.arg, st)
        if roll is not None:
            if kind != "f32":
                raise PaigError(f"decoder fwd: the merged rollout launch takes fp32 targets, not {kind}")
            return self._fn("fwd_rollout")(*roll, *dec)
        return self._fn("fwd_t8" if kind == "u8" else "fwd")(*dec)

    @property
    def slab_len(self):
        """Floats per slab row of the backward's partial source gradients."""
        return int(self.L.paig_decoder_slab_len(*self.shape))

    def bwd_sizes(self, F, grp=0, live=0):
        """(slab rows, scratch floats) of bwd over F frames grouped by grp of
        which the first `live` per group carry a loss weight (0: all)."""
        if self.sigma.on_device:
            return (self.L.paig_decoder_bwd_blocks_sigma_dev(F, *self.shape),
                    self.L.paig_decoder_bwd_scratch_sigma_dev(F, *self.shape))
        return (self.L.paig_decoder_bwd_blocks_sigma(F, grp, live, *self.shape, self.sigma.value),
                self.L.paig_decoder_bwd_scratch_sigma(F, *self.shape, self.sigma.value))

    def bwd(self, pos_view, targets, dsse, lw, dout, dout_fs, dpos, slab, scratch, F, live, st, dsig=None):
        """Position gradients (dpos) and partial source gradients (slab rows:
        bwd_sizes) of F frames.  The SSE's per-frame weights are the array
        dsse, or formed in-kernel from lw = (mode, LossAdjoints); dout: a dense
        dL/dout (or None).  Without targets the gradient is dout alone.  dsig
        (device sigma only): every frame's dL/dsigma, fp64."""
        kind = targets.kind
        if dsse is not None and lw is not None:
            raise PaigError("decoder bwd: both a weight array and in-kernel loss weights")
        if kind == "none":
            if dsse is not None or lw is not None:
                raise PaigError("decoder bwd: loss weights without targets")
            if dout is None:
                raise PaigError("decoder bwd: neither targets nor a dense dL/dout")
            # the target pointer must still address F valid frames: dout does
            targets = Targets.frames(dout, dout_fs, 0, 0)
        if dsig is not None and not self.sigma.has_grad:
            raise PaigError("decoder bwd: dL/dsigma needs a device-resident sigma")
        if lw is not None:
            mode, adj = lw
            lwa = (mode, ptr(adj.dt), ptr(adj.de), ptr(adj.dr), float(adj.ae), adj.B, adj.Te, adj.R, adj.pred)
        else:
            lwa = (0, None, None, None, 0.0, 0, 0, 0, 0)
        tail = (self.sigma.arg, dsig, st) if self.sigma.on_device else (self.sigma.arg, st)
        return self._fn("bwd_ex")(*pos_view, *self.sources, *targets, dsse, *lwa, dout, dout_fs, dpos, slab, scratch,
                                  F, live, *self.shape, *tail)

    def parts(self, pos, inner, contents, masks, F, st):
        """The per-object intermediates (K warped contents + background, K + 1
        masks, each [F][3][H][W]) of F frames at pos + f * inner."""
        return self._fn("parts")(pos, inner, *self.sources, contents, masks, F, *self.shape, self.sigma.arg, st)
