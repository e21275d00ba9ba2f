"""The rollout cells' C-ABI calls, described and packed in one place.

Every cell takes (pos0, vel0) to pvs [B][R + 1][2D] and back, on one of three
kernel families.  SPECS states each cell once; every caller above it (the
engine, the standalone cell module, PhysicsNet's flat parameter buffer) goes
through SPECS and RolloutOps, which picks the export and lays out its
positional arguments.  A new cell is one SPECS entry (and, for a new kernel
family, one Family).

Pure Python: nothing here allocates, reads the environment or touches torch
beyond ptr(); every device operand is an address (int, or None for NULL),
except the cell's own parameters and the saved-activation workspace (a tensor
or None: its size travels with it).
"""
from typing import Callable, NamedTuple

from ._lib import PaigError, ptr


class Family(NamedTuple):
    """The exports of one kernel family and its probe tags (None: unlabelled)."""
    fwd: str
    bwd: str
    workspace: str = None    # the saved-activation size query (bytes); None: the backward reads pvs alone
    probe_fwd: str = None
    probe_bwd: str = None


PHYSICS = Family("paig_rollout_fwd", "paig_rollout_bwd")
LSTM = Family("paig_rollout_lstm_fwd", "paig_rollout_lstm_bwd", "paig_rollout_lstm_workspace",
              "rollout_lstm_fwd", "rollout_lstm_bwd")
INTERACTION = Family("paig_rollout_in_fwd", "paig_rollout_in_bwd", "paig_rollout_in_workspace",
                     "rollout_in_fwd", "rollout_in_bwd")


def _never(need_saved, grad_mode):
    return False


class CellSpec(NamedTuple):
    kind: int                # the class's KIND (PHYSICS: paig_rollout_fwd's cell argument)
    family: Family
    operands: Callable       # cell -> its operands in the kernels' argument order: (dt, p0, p1) / weights()
    names: tuple             # trainable parameters under "rollout_cell.", in flat-buffer (and gradient-argument) order
    bwd_reads: tuple = ()    # learned cells: which of the operands the backward takes
    saves: Callable = _never   # (need_saved, grad_mode) -> whether the engine's forward allocates the workspace
    units_ctor: bool = False   # the constructor takes (recurrent_units, half) after the two sizes


def _weights(cell):
    return cell.weights()


SPECS = {
    "spring_ode_cell": CellSpec(0, PHYSICS, lambda c: (c.dt, c.k, c.equil), ("k", "equil")),
    "bouncing_ode_cell": CellSpec(1, PHYSICS, lambda c: (c.dt, None, None), ()),
    "gravity_ode_cell": CellSpec(2, PHYSICS, lambda c: (c.dt, c.g, c.m), ("g",)),
    # the opt-in split-size-2 cells
    "spring2d_ode_cell": CellSpec(3, PHYSICS, lambda c: (c.dt, c.k, c.equil), ("k", "equil")),
    "bouncing2d_ode_cell": CellSpec(4, PHYSICS, lambda c: (c.dt, None, None), ()),
    # the learned cells: fp32, no dt; their names close the fp32 buffer's late part, after every other name
    "lstm_ode_cell": CellSpec(
        5, LSTM, _weights,
        ("lstm.weight_ih", "lstm.weight_hh", "lstm.bias_ih", "lstm.bias_hh", "proj.weight", "proj.bias"),
        bwd_reads=(0, 1, 4), units_ctor=True,
        saves=lambda need_saved, grad_mode: need_saved),   # what BPTT reads; inference saves nothing
    "interaction_ode_cell": CellSpec(
        6, INTERACTION, _weights,
        ("rel.0.weight", "rel.0.bias", "rel.2.weight", "rel.2.bias", "obj.0.weight", "obj.0.bias", "obj.2.weight",
         "obj.2.bias"),
        bwd_reads=(0, 2, 4, 6), units_ctor=True,
        saves=lambda need_saved, grad_mode: need_saved and grad_mode),   # not under no_grad (an evaluation forward)
}


class RolloutOps:
    """The rollout calls of one cell module over B sequences of D coordinates
    and R steps on the library L; half: the learned cells' position scale
    (frame side / 2)."""

    def __init__(self, L, cell, B, D, R, half):
        self.L, self.cell, self.spec = L, cell, SPECS[type(cell).__name__]
        self.B, self.D, self.R, self.half = B, D, R, half

    @property
    def learned(self):
        """Whether the backward reads a workspace its forward saved (else pvs alone)."""
        return self.spec.family.workspace is not None

    def _shape(self):
        return (self.B, self.D, self.cell.recurrent_units, self.R) if self.learned else (self.B, self.D, self.R)

    def workspace_floats(self):
        """Floats of the workspace the forward saves for its backward (0: none)."""
        if not self.learned:
            return 0
        return getattr(self.L, self.spec.family.workspace)(*self._shape()) // 4

    def part_doubles(self):
        """Doubles of the physics backward's block partials (0: a learned cell)."""
        return 0 if self.learned else 2 * self.L.paig_rollout_bwd_blocks(self.B)

    def merged_args(self, pos0, ld, vel0, pvs):
        """(cell, pos0, ld, vel0, dt, p0, p1, pvs, B, D, R): paig_rollout_fwd's
        arguments, which DecoderOps.fwd(roll=...) runs in the decode's launch."""
        if self.learned:
            raise PaigError(f"{type(self.cell).__name__}: only the physics rollout shares the decoder's launch")
        dt, p0, p1 = self.spec.operands(self.cell)
        return (self.spec.kind, pos0, ld, vel0, ptr(dt), ptr(p0), ptr(p1), pvs, *self._shape())

    def fwd(self, pos0, ld, vel0, pvs, ws, st):
        """All R steps from pos0 (row stride ld) and vel0 ([n_objs][B][2], or
        None) into pvs, one launch; ws: the workspace tensor the backward will
        read, or None (inference)."""
        if not self.learned:
            return self.L.paig_rollout_fwd(*self.merged_args(pos0, ld, vel0, pvs), st)
        return getattr(self.L, self.spec.family.fwd)(
            pos0, ld, vel0, *[ptr(w) for w in self.spec.operands(self.cell)], self.half, pvs, ptr(ws),
            ws.numel() * 4 if ws is not None else 0, *self._shape(), st)

    def bwd(self, pvs, dpos_roll, dpvs, dpos0, dvel0, grads, part, ws, accumulate, st):
        """d pos0 and d vel0 from the adjoints of the rolled-out positions
        (dpos_roll [B][R][D]) and of pvs (dpvs), either None.  grads: where each
        of spec.names' gradients goes, in that order (physics: (gk, gq), fp64,
        padded with NULL; part: its block partials, part_doubles())."""
        if not self.learned:
            dt, p0, p1 = self.spec.operands(self.cell)
            gk, gq = (*grads, None, None)[:2]
            return self.L.paig_rollout_bwd(self.spec.kind, pvs, dpos_roll, dpvs, ptr(dt), ptr(p0), ptr(p1), dpos0,
                                           dvel0, part, gk, gq, accumulate, *self._shape(), st)
        W = self.spec.operands(self.cell)
        return getattr(self.L, self.spec.family.bwd)(
            dpos_roll, dpvs, *[ptr(W[i]) for i in self.spec.bwd_reads], self.half, dpos0, dvel0, *grads, accumulate,
            ptr(ws), ws.numel() * 4, *self._shape(), st)
