"""Physics cells, mirroring nn/network/cells.py of the reference: same
classes, the same RNNCell base (its unused weight_ih/weight_hh/bias_* stay in
the state_dict and the init RNG stream, quirk Q8) and the same parameters
(dt fp32 frozen; k, equil / g, m 0-dim fp64, quirk Q9).

The integrators themselves run fused over all rollout steps in the HIP kernel
``paig_rollout_fwd/bwd`` (csrc/rollout.hip), which restates
spring (:31-51), bouncing (:60-83) and gravity (:96-106) exactly, including
the split-size-1 quirk Q3.  Gravity recomputes A = exp(g) exp(2m) per step
(the reference computes it once in __init__, Q4).

spring2d_ode_cell / bouncing2d_ode_cell (rollout kinds 3 / 4) are the opt-in
fix of Q3: the same cells with split size 2, two objects in the plane.

lstm_ode_cell is the black-box baseline (not in the reference, whose "lstm"
table entry its rollout cannot call): a learned LSTM step in the place of the
equations, on paig_rollout_lstm_fwd/bwd (csrc/rollout_lstm.hip).

interaction_ode_cell is the object-centric learned baseline (not in the
reference either): an interaction network, one relation MLP shared by all
ordered pairs of objects and one object MLP shared by all objects, on
paig_rollout_in_fwd/bwd (csrc/rollout_in.hip)."""
import numpy as np
import torch
import torch.nn as tnn


def _forward(self, poss, vels):
    """One cell step (the physics cells: 5 substeps) on the cell's rollout
    kernels with R = 1: poss, vels [B, coord_units/2] -> (poss, vels).  The
    training path runs all R steps in one launch instead (PhysicsNet.forward)."""
    from paig_reproduction_amd.nn.network import native_modules as _nm
    return _nm.cell_forward(self, poss, vels)


class ode_cell(tnn.RNNCell):
    def __init__(self, input_size, hidden_size):
        super().__init__(input_size, hidden_size)
        self.input_size = input_size
        self.hidden_size = hidden_size

    @property
    def state_size(self):
        return self.hidden_size, self.hidden_size

    def zero_state(self, batch_size, dtype):
        x_0 = torch.zeros(batch_size, self.hidden_size, dtype=dtype)
        v_0 = torch.zeros(batch_size, self.hidden_size, dtype=dtype)
        return x_0, v_0

    forward = _forward


class spring_ode_cell(ode_cell):
    """ Assumes there are 2 objects """
    KIND = 0

    def __init__(self, input_size, hidden_size):
        super().__init__(input_size, hidden_size)
        self.dt = tnn.Parameter(torch.tensor(0.3), requires_grad=False)
        self.k = tnn.Parameter(torch.tensor(np.log(1.0)), requires_grad=True)
        self.equil = tnn.Parameter(torch.tensor(np.log(1.0)), requires_grad=True)


class bouncing_ode_cell(ode_cell):
    """ Assumes there are 2 objects """
    KIND = 1

    def __init__(self, input_size, hidden_size):
        super().__init__(input_size, hidden_size)
        self.dt = tnn.Parameter(torch.tensor(0.3), requires_grad=False)


class spring2d_ode_cell(spring_ode_cell):
    """Opt-in (not the reference's behaviour): spring_ode_cell with split
    size 2.  The two objects (x0, y0) and (x1, y1) are joined by a vector
    spring, F = exp(k) (|d| - 2 exp(equil)) d / |d| with d = p0 - p1: the
    physics nn/datasets/synth.py renders.  Same parameters, creation order,
    state_dict and init RNG stream as spring_ode_cell."""
    KIND = 3


class bouncing2d_ode_cell(bouncing_ode_cell):
    """Opt-in (not the reference's behaviour): bouncing_ode_cell with split
    size 2.  All four coordinates move and bounce off the walls 0 and 32
    (radius 2); no ball-to-ball collisions, as in the reference."""
    KIND = 4


class gravity_ode_cell(ode_cell):
    """ Assumes there are 3 objects """
    KIND = 2

    def __init__(self, input_size, hidden_size):
        super().__init__(input_size, hidden_size)
        self.dt = tnn.Parameter(torch.tensor(0.5), requires_grad=False)
        self.g = tnn.Parameter(torch.tensor(np.log(1.0)), requires_grad=True)
        self.m = tnn.Parameter(torch.tensor(np.log(1.0)), requires_grad=False)

    @property
    def A(self):
        return torch.exp(self.g.detach()) * torch.exp(2 * self.m.detach())


class lstm_ode_cell(tnn.Module):
    """The black-box rollout cell: no equation, no dt.  One step is

        x = [(pos - s) / s, vel / s]              s = frame side / 2
        h, c = LSTMCell(x, (h, c))                h = c = 0 at the start of every rollout
        y = proj(h);  pos += s y[:D];  vel += s y[D:]

    with lstm = nn.LSTMCell(2D, H) and proj = nn.Linear(H, 2D), D =
    input_size.  Torch's default initialisation; proj is scaled by 0.1, so a
    fresh cell moves objects by about a pixel per step."""
    KIND = 5   # no kind of the physics kernels: a family of its own (rollout_ops.LSTM)
    H_MAX = 128

    def __init__(self, input_size, hidden_size, recurrent_units=100, half=16.0):
        super().__init__()
        H = recurrent_units
        if isinstance(H, bool) or not isinstance(H, int) or H % 4 != 0 or not 4 <= H <= self.H_MAX:
            raise ValueError(f"lstm_ode_cell: recurrent_units={H!r} must be a multiple of 4 in [4, {self.H_MAX}]")
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.recurrent_units = H
        self.half = float(half)
        self.lstm = tnn.LSTMCell(2 * input_size, H)
        self.proj = tnn.Linear(H, 2 * input_size)
        with torch.no_grad():
            self.proj.weight.mul_(0.1)
            self.proj.bias.mul_(0.1)

    def weights(self):
        """(W_ih, W_hh, b_ih, b_hh, W_p, b_p), the kernels' argument order."""
        return (self.lstm.weight_ih, self.lstm.weight_hh, self.lstm.bias_ih, self.lstm.bias_hh, self.proj.weight,
                self.proj.bias)

    forward = _forward   # (from a zero hidden state)


class interaction_ode_cell(tnn.Module):
    """The interaction-network rollout cell: no equation, no dt, no hidden
    state.  With K = input_size / 2 objects, s = frame side / 2 and
    pos_i = pos[:, 2i:2i+2] (vel_i likewise), one step is

        s_i  = [(pos_i - s) / s, vel_i / s]
        e_ij = rel([s_i, s_j])                    every ordered pair j != i (receiver first)
        a_i  = sum_{j != i} e_ij                  in increasing j
        y_i  = obj([s_i, a_i]);  pos_i += s y_i[:2];  vel_i += s y_i[2:]

    with rel = Linear(8, H), Tanh, Linear(H, H), Tanh and obj = Linear(4 + H,
    H), Tanh, Linear(H, 4).  Torch's default initialisation; obj's last layer
    is scaled by 0.1, so a fresh cell moves objects by about a pixel per
    step.  Permutation-equivariant in the objects by construction."""
    KIND = 6   # no kind of the physics kernels: a family of its own (rollout_ops.INTERACTION)
    H_MAX = 128

    def __init__(self, input_size, hidden_size, recurrent_units=100, half=16.0):
        super().__init__()
        H = recurrent_units
        if isinstance(H, bool) or not isinstance(H, int) or H % 4 != 0 or not 4 <= H <= self.H_MAX:
            raise ValueError(f"interaction_ode_cell: recurrent_units={H!r} must be a multiple of 4 in [4, {self.H_MAX}]")
        if input_size not in (4, 6):
            raise ValueError(f"interaction_ode_cell: input_size={input_size!r}, 2 or 3 objects in the plane (4 or 6)")
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.recurrent_units = H
        self.half = float(half)
        self.rel = tnn.Sequential(tnn.Linear(8, H), tnn.Tanh(), tnn.Linear(H, H), tnn.Tanh())
        self.obj = tnn.Sequential(tnn.Linear(4 + H, H), tnn.Tanh(), tnn.Linear(H, 4))
        with torch.no_grad():
            self.obj[2].weight.mul_(0.1)
            self.obj[2].bias.mul_(0.1)

    def weights(self):
        """(W_r1, b_r1, W_r2, b_r2, W_o1, b_o1, W_o2, b_o2), the kernels' argument order."""
        return (self.rel[0].weight, self.rel[0].bias, self.rel[2].weight, self.rel[2].bias, self.obj[0].weight,
                self.obj[0].bias, self.obj[2].weight, self.obj[2].bias)

    forward = _forward
