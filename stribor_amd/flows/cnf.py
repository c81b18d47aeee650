"""Continuous normalizing flow (reference: stribor/flows/cnf.py:13-262): ``ContinuousTransform``.

Same constructor, methods and ``state_dict`` keys (``odefunc.diffeq.net.net.0.weight``, ..., ``odefunc._num_evals``).  The solve
runs on a FIXED grid with ``solver='euler' | 'midpoint' | 'rk4'`` (torchdiffeq 0.2.2's fixed-grid family; ``rk4`` is the 3/8
rule), or under ``solver='dopri5_per_sample'`` with error control to ``atol`` / ``rtol``; the reference's adaptive and Adams solver
names are accepted -- they are its defaults and checkpoints must load -- and raise ``NotImplementedError`` when evaluated (DESIGN.md
"CNF").

``'dopri5_per_sample'`` is Dormand-Prince 5(4) with ONE STEP-SIZE CONTROLLER PER SAMPLE (a row; under ``set_data`` a set): the error
norm is taken over the sample's own entries, so its result does not depend on its batch, and the last step lands on T exactly -- two
deliberate differences from torchdiffeq's ``dopri5``, which is why that name still raises.  In the dense tier's setting without a
graph, a ``DiffeqMLP`` with dim <= 32, 1 + dim + latent <= 128 and hidden layers of <= 64 units is ONE launch of
``sx_cnf_adaptive_flow`` (time is the net's first input column, so every row of a tile carries its own time).  Sets, masks, calls
that want a graph, training mode and the other five tiers' nets all run the same controller as torch ops for now
(``_solve_composed_adaptive``; with a graph: through the accepted steps, step sizes frozen).  ``last_solver_stats`` holds (accepted,
rejected, status) per sample.

Without an autograd graph, a ``DiffeqMLP`` with one or two hidden layers is ONE launch of ``sx_cnf_flow``: the state, the stage
vectors and the log-det accumulator stay in registers for the whole grid, the weights sit in LDS, and the exact divergence comes
from a closed form whose weight-only constants (``trace_constants``) are derived once in fp64.  Everything else -- other nets,
``mask``, ``set_data``, and every other call that has to build a graph -- runs the same grid and tableau as a loop of torch ops over
the module (``_solve_composed``); gradients are those of the discretised steps.

Training with the default ``divergence='approximate'`` (training mode, no mask, no sets) over a ``DiffeqMLP`` with hidden layers of
<= 32 units, dim <= 32 and 1 + dim + latent <= 64 runs on two kernels: ``sx_cnf_train_fwd`` (the solve with Hutchinson's estimate for
the noise drawn once per solve, plus one checkpoint per step) and ``sx_cnf_train_bwd`` (the discrete adjoint of the same grid and
tableau, weight gradients contracted in-kernel and summed in a fixed order); ``hutchinson_closed_form`` states one evaluation and its
adjoints in torch (DESIGN.md "CNF", training on the kernel).

Sets of shape (..., N, dim): a ``net.DiffeqDeepset`` over a ``net.EquivariantNet`` (one or two hidden layers of <= 64 units, N <= 128,
dim <= 32, 1 + dim + latent <= 64, no final activation) under ``set_data=True`` / ``divergence='compute_set'`` (or ``'none'``) is ONE
launch of ``sx_cnf_set_flow`` under the same conditions: the per-element share of the set's divergence -- what
``divergence_exact_for_sets(...).sum(-1)`` gives with N * dim reverse passes per evaluation -- comes from a closed form whose
weight-only constants (``set_trace_constants``; they depend on N) are derived once per N in fp64 (DESIGN.md "CNF on sets").

``divergence='exact'`` over a ``net.DiffeqExactTraceMLP`` (two MADEs + a dimwise MLP, one or two hidden layers of <= 64 units,
dim <= 16, d_h <= 8, latent <= 64) is ONE launch of ``sx_cnf_exact_flow`` under the same conditions: the masked weights are staged
into the kernel's LDS image once (cached, guarded on weights and masks) and the Jacobian diagonal is a forward-mode tangent beside the
value.  Over a ``net.DiffeqExactTraceDeepSet`` on sets (..., N, dim) (N <= 128, the same widths, sum / mean / max pooling) it is ONE
launch of ``sx_cnf_exact_set_flow``: the same image scheme plus one ordered exchange through LDS per evaluation for the exclusive
pooling.  Over a ``net.diffeq_exact_trace.DiffeqExactTraceAttention`` on sets (hidden_dims [E] or [H1, E] with H1 <= 64 and E <= 32, dim <= 8, at most four
query tiles, 1, 2 or 4 heads, d_h <= 8, latent <= 64, N <= 128) it is ONE launch of ``sx_cnf_exact_attn_flow``: keys and values meet in
LDS once per evaluation, dim attentions with the MADE's per-dimension queries run against them, and the trace is the dimwise net's
tangent -- no tangent attention, where ``sx_cnf_attn_flow`` pays 1 + dim attentions for it.  Any other net under
'exact' runs the composition path over ``net.FuncAndDiagJac``.

Sets under ``set_data=True`` / ``divergence='compute_set'`` (or ``'none'``) over a ``net.DiffeqSelfAttention`` (embeddings of one or two
Linear layers, hidden <= 64, embedding <= 32, 1, 2 or 4 heads, N <= 128, dim <= 8, dim + latent <= 32) are ONE launch of
``sx_cnf_attn_flow``: keys and values meet in LDS once per evaluation, and the per-element divergence comes from a forward tangent per
coordinate (``net.self_attention_closed_form`` states it in torch) -- 1 + dim attentions per evaluation where
``divergence_exact_for_sets`` makes N * dim reverse passes (DESIGN.md "CNF on sets with attention").

How a call picks its kernel is ``ContinuousTransform._choose`` over the table ``_TIERS``, in the order dense, exact-trace sets,
exact-trace attention sets, exact-trace, sets, attention sets, after the training pair and before the composition path; ``_solve`` has one tail for every route.
One planner per kernel (``_kernel_net``, ``_train_kernel_net``, ``_set_kernel_net``, ``_attn_kernel_net``, ``_exact_kernel_net``,
``_exact_set_kernel_net``, ``_exact_attn_kernel_net``) returns (net descriptor, keep-alive list) or None; the conditions they share -- the activation, the
tensors, the ``Linear (act Linear)*`` stack, the tile count -- and the activations' derivatives are ``net.cover``'s.  ``Grid`` carries
a solve's (solver, step, points) and yields the launches' common argument tail.
"""
import ctypes
from typing import Callable, Dict, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from ..flow import Transform, flatten_rows, graph_wanted
from ..fused import ProgramCache
from ..net import cover, diffeq_exact_trace as exact_trace
from ..net.attention import SelfAttention
from ..net.diffeq import DiffeqDeepset, DiffeqMLP, DiffeqSelfAttention
from ..net.diffeq_zero_trace import DiffeqZeroTraceAttention, DiffeqZeroTraceDeepSet
from ..net.equivariant import EquivariantLayer, EquivariantNet
from ..net.mlp import MLP
from ..util.divergence import divergence_approx, divergence_exact, divergence_exact_for_sets

__all__ = ['ContinuousTransform']

FIXED_SOLVERS = ('euler', 'midpoint', 'rk4')
ADAPTIVE_SOLVERS = ('dopri5_per_sample',)
STAGES = {'euler': 1, 'midpoint': 2, 'rk4': 4}
MAX_NUM_STEPS = 4096          # attempts per sample before an adaptive solve gives up: a safety cap, not a tuned value


def _r32(v: float) -> float:
    """The fp32 rounding of an fp64 value, as a Python float (tensor * float then multiplies by exactly that fp32 number)."""
    return float(np.float32(v))


class DormandPrince(NamedTuple):
    """The Dormand-Prince 5(4) tableau of 'dopri5_per_sample' (DESIGN.md "CNF") in fp64: a[i] = the weights of k1 .. k_i in the input
    of stage i + 1 (a[6] = b: FSAL), the nodes c, the solution weights b and the error weights e = b - b*."""
    a: tuple
    c: tuple
    b: tuple
    e: tuple


def _dormand_prince() -> DormandPrince:
    b = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.0)
    b_star = (5179 / 57600, 0.0, 7571 / 16695, 393 / 640, -92097 / 339200, 187 / 2100, 1 / 40)
    a = ((), (1 / 5,), (3 / 40, 9 / 40), (44 / 45, -56 / 15, 32 / 9), (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
         (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656), b[:6])
    return DormandPrince(a, (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0), b, tuple(p - q for p, q in zip(b, b_star)))


DOPRI5 = _dormand_prince()
_DIVERGENCES = ('compute', 'compute_set', 'approximate', 'exact', 'none')


class Grid(NamedTuple):
    """The fixed grid of one solve: the solver's name, the step size (None: the single step) and the fp32 points of `fixed_grid`."""
    name: str
    step: Optional[float]
    points: np.ndarray

    def c_args(self, n: int):
        """The arguments every launch ends its solve with: rows, solver code, steps, t0, t1 and the step size (0: one step)."""
        return n, _hip.CNF_SOLVERS[self.name], len(self.points) - 1, float(self.points[0]), float(self.points[-1]), float(self.step or 0.0)


def fixed_grid(t0: float, t1: float, step_size: Optional[float] = None) -> np.ndarray:
    """The time grid of a fixed-step solve as fp32 points (the solver specification, DESIGN.md "CNF"): without `step_size` the
    single step [t0, t1]; with it ceil(|t1 - t0| / step_size + 1) points t0 +- i * step_size, the last one replaced by t1.  All
    arithmetic is fp32, as the reference solver's is on fp32 integration times."""
    f = np.float32
    t0, t1 = f(t0), f(t1)
    if step_size is None:
        return np.array([t0, t1], dtype=f)
    h = f(step_size)
    if not h > 0:
        raise ValueError(f'step_size must be positive (got {step_size})')
    n = int(np.ceil(f(f(abs(f(t1 - t0))) / h) + f(1)))
    sgn = f(-1.0) if t1 < t0 else f(1.0)
    grid = (t0 + sgn * (np.arange(n, dtype=f) * h)).astype(f)
    grid[-1] = t1
    return grid


def trace_constants(weights, dim: int):
    """The weight-only constants of tr df/dx for f = MLP([t, x, latent]) without a final activation, W1x = the x columns
    1 .. dim of the first weight:  one hidden layer: c [H1], c_j = sum_i W2[i, j] W1x[j, i];  two: C [H2, H1],
    C[k, j] = W2[k, j] (W1x W3)[j, k].  Then tr J = sum_j d1_j c_j, resp. d2^T C d1, with d_l = act'(hidden layer l).
    fp64 in, fp64 out (the caller rounds once)."""
    W1x = weights[0][:, 1:1 + dim]
    if len(weights) == 2:
        return (weights[1].t() * W1x).sum(-1)
    W2, W3 = weights[1], weights[2]
    return W2 * (W1x @ W3).t()


def set_trace_constants(weights, dim: int, n: int):
    """The weight-only constants of the per-element divergence of f = EquivariantNet([t, x, latent]) over sets of n elements, no
    final activation.  `weights`: per layer (A_l, B_l) = (l1.weight, l2.weight).  With E1 = A_1[:, 1 : 1 + dim], F1 = B_1[:, 1 : 1 +
    dim] / n, G_l = B_l / n, c(P, Q)_h = sum_a P[a, h] Q[h, a] and C(Q, R, P) = Q o (R P)^T (elementwise, [H2, H1]):
      one hidden layer: [2, H1] = (c_d, c_s), c_d = c(A2, E1 + F1) + c(G2, E1), c_s = c(G2, F1);
          tr_i = d1_i . c_d + s1 . c_s
      two: [5, H2, H1] = (C_abd, C_c, C_e, C_f, C_g), C_abd = C(A2, E1 + F1, A3) + C(G2, E1, A3) + C(A2, E1, G3),
          C_c = C(G2, F1, A3), C_e = C(A2, F1, G3), C_f = C(G2, E1, G3), C_g = C(G2, F1, G3);
          tr_i = d2_i^T C_abd d1_i + d2_i^T C_c s1 + s2^T C_f d1_i + [sum_j d2_j^T C_e d1_j + s2^T C_g s1]
    with d_l,i = act'(hidden layer l of element i) and s_l = sum_j d_l,j over the set.  fp64 in, fp64 out (the caller rounds once)."""
    (A1, B1), (A2, B2) = weights[0], weights[1]
    E1, F1, G2 = A1[:, 1:1 + dim], B1[:, 1:1 + dim] / n, B2 / n
    if len(weights) == 2:
        c = lambda P, Q: (P.t() * Q).sum(-1)
        return torch.stack([c(A2, E1 + F1) + c(G2, E1), c(G2, F1)])
    A3, G3 = weights[2][0], weights[2][1] / n
    C = lambda Q, R, P: Q * (R @ P).t()
    return torch.stack([C(A2, E1 + F1, A3) + C(G2, E1, A3) + C(A2, E1, G3), C(G2, F1, A3), C(A2, F1, G3), C(G2, E1, G3), C(G2, F1, G3)])


def _act_and_derivatives(name: str, a):
    """(act(a), act'(a), act''(a)) with both derivatives taken from the activation's OUTPUT, as the kernels take them."""
    if name not in cover.ACTS:
        raise ValueError(f'no closed form for activation {name!r}')
    act, first, second = cover.ACTS[name]
    h = act(a)
    d = first(h)
    return h, d, second(h, d)


def hutchinson_closed_form(weights, biases, activation: str, t, z, e, latent=None, k_bar=None, q_bar=None):
    """One evaluation of the training CNF in torch ops, as ``sx_cnf_train_fwd`` / ``sx_cnf_train_bwd`` compute it (any dtype and
    device): f = MLP([t, z, latent]) with one or two hidden layers and no final activation, and Hutchinson's estimate q = e^T (df/dz) e
    for a fixed noise row e, without autograd -- u1 = W1x e and v = W_last^T e are constant along a solve, d = act', s = act'':
      one hidden layer:  q = sum d1 u1 v;      two:  w = d1 u1, r = W2 w, q = sum v d2 r.
    -> (k, q [...]).  With the adjoints `k_bar` [..., dim] and `q_bar` [...] also a dict: 'z', 'latent' (None without latent) and 'W',
    'b' (lists, one entry per Linear layer, summed over the rows) -- the reverse pass of the two values, i.e. what
    ``autograd.grad(..., create_graph=True)`` followed by a second differentiation gives."""
    D = z.shape[-1]
    W1 = weights[0]
    W1x, W1l, Wl = W1[:, 1:1 + D], W1[:, 1 + D:], weights[-1]
    zero = lambda W: torch.zeros(W.shape[0], dtype=z.dtype, device=z.device)
    bs = [zero(W) if b is None else b for W, b in zip(weights, biases)]
    u1, v = e @ W1x.t(), e @ Wl
    a1 = z @ W1x.t() + bs[0] + t * W1[:, 0]
    if latent is not None:
        a1 = a1 + latent @ W1l.t()
    h1, d1, s1 = _act_and_derivatives(activation, a1)
    if len(weights) == 2:
        k = h1 @ Wl.t() + bs[1]
        q = (d1 * u1 * v).sum(-1)
    else:
        W2 = weights[1]
        h2, d2, s2 = _act_and_derivatives(activation, h1 @ W2.t() + bs[1])
        k = h2 @ Wl.t() + bs[2]
        w = d1 * u1
        r = w @ W2.t()
        q = (v * d2 * r).sum(-1)
    if k_bar is None:
        return k, q
    qb = q_bar.unsqueeze(-1)
    rows = lambda m: m.reshape(-1, m.shape[-1])
    outer = lambda a, b: rows(a).t() @ rows(b)
    if len(weights) == 2:
        a1b = (k_bar @ Wl) * d1 + qb * s1 * u1 * v
        u1b, vb = qb * d1 * v, qb * d1 * u1
        gW = [None, outer(k_bar, h1) + outer(e, vb)]
        gb = [None, rows(k_bar).sum(0)]
    else:
        rb = qb * v * d2
        a2b = (k_bar @ Wl) * d2 + qb * s2 * v * r
        vb = qb * d2 * r
        wb = rb @ W2
        a1b = (a2b @ W2) * d1 + wb * s1 * u1
        u1b = wb * d1
        gW = [None, outer(a2b, h1) + outer(rb, w), outer(k_bar, h2) + outer(e, vb)]
        gb = [None, rows(a2b).sum(0), rows(k_bar).sum(0)]
    cols = [torch.full_like(z[..., :1], 1.0) * t, z] + ([] if latent is None else [latent])
    gW[0] = outer(a1b, torch.cat(cols, -1))
    gW[0][:, 1:1 + D] += outer(u1b, e)
    gb[0] = rows(a1b).sum(0)
    return k, q, {'z': a1b @ W1x, 'latent': None if latent is None else a1b @ W1l, 'W': gW, 'b': gb}


class _CNFTrain(torch.autograd.Function):
    """(y, ldj) = the Hutchinson solve of sx_cnf_train_fwd with checkpoints; backward: sx_cnf_train_bwd, the discrete adjoint of the
    same grid and tableau, weight gradients contracted in-kernel.  Differentiable once."""

    @staticmethod
    def forward(ctx, module, name, step, grid, x2, lat2, e2, *params):
        n_steps = len(grid) - 1
        ckpt = torch.empty(n_steps, *x2.shape, dtype=torch.float32, device=x2.device)
        y, ldj = module._train_forward(x2, lat2, e2, name, step, grid, ckpt)
        ctx.module, ctx.grid = module, Grid(name, step, grid)
        ctx.has_latent = lat2 is not None
        ctx.save_for_backward(ckpt, e2, *( [lat2] if lat2 is not None else []), *[p for p in params if p is not None])
        ctx.bias_mask = [p is not None for p in params]
        return y, ldj

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, gldj):
        module = ctx.module
        saved = list(ctx.saved_tensors)
        ckpt, e2 = saved[0], saved[1]
        lat2 = saved[2] if ctx.has_latent else None
        n, dim = e2.shape
        need = ctx.needs_input_grad
        plan = module._train_kernel_net(0 if lat2 is None else lat2.shape[-1], e2.device)
        if plan is None:
            raise RuntimeError('stribor_amd: the CNF changed between the forward and the backward of a training step')
        d, keep = plan
        gy = gy.to(torch.float32).contiguous()
        gldj = gldj.to(torch.float32).reshape(-1).contiguous()
        gx = torch.empty_like(gy)
        glat = torch.empty_like(lat2) if lat2 is not None and need[5] else None
        partial = torch.empty(max(1, _hip.lib().sx_cnf_train_partial_floats(d, n)), dtype=torch.float32, device=e2.device)
        grads = _hip.sx_cnf_train_grads()
        out = []
        for i in range(d.n_layers):
            W = keep[2 * i]
            gW = torch.empty_like(W) if need[7 + 2 * i] else None
            gb = torch.empty_like(keep[2 * i + 1]) if ctx.bias_mask[2 * i + 1] and need[8 + 2 * i] else None
            grads.dW[i], grads.db[i] = _hip.ptr(gW), _hip.ptr(gb)
            out += [gW, gb]
        _hip.call('sx_cnf_train_bwd', e2, ctypes.byref(d), ckpt.data_ptr(), _hip.ptr(lat2), e2.data_ptr(), gy.data_ptr(), gldj.data_ptr(),
                  gx.data_ptr(), _hip.ptr(glat), partial.data_ptr(), ctypes.byref(grads), *ctx.grid.c_args(n))
        del keep
        return (None, None, None, None, gx if need[4] else None, glat, None, *out)


class ODEfunc(nn.Module):
    """The augmented dynamics of cnf.py:13-99: d/dt (x, a) = (f(t, x), -div f), with a kept per feature."""

    def __init__(self, diffeq, divergence=None, rademacher=False, has_latent=False, set_data=False, **kwargs):
        super().__init__()
        assert divergence in _DIVERGENCES
        self.diffeq = diffeq
        self.rademacher = rademacher
        self.divergence = divergence
        self.has_latent = has_latent
        self.set_data = set_data
        self.register_buffer('_num_evals', torch.tensor(0.))
        self._e = None

    def before_odeint(self, e=None):
        self._e = e
        self._num_evals.fill_(0)

    def num_evals(self):
        return self._num_evals.item()

    def exact_trace(self) -> bool:
        """Does this setting evaluate the exact divergence of a row-wise net (cnf.py:91-95)?"""
        return not self.set_data and (self.divergence == 'compute' or (self.divergence == 'approximate' and not self.training))

    def exact_set_trace(self) -> bool:
        """Does this setting evaluate the exact divergence of a set net (cnf.py:91-93: divergence_exact_for_sets)?"""
        if self.divergence == 'compute_set':
            return True
        return self.set_data and (self.divergence == 'compute' or (self.divergence == 'approximate' and not self.training))

    def forward(self, t, states):
        """states = (x, a[, latent][, mask]) -> their time derivatives (zeros for latent and mask)."""
        y = states[0]
        t = torch.as_tensor(t)
        # (one time for all, or -- an adaptive solve -- one per sample, shaped to broadcast against y[..., :1])
        t = (t.reshape(1) if t.numel() == 1 else t).to(y)
        latent = mask = None
        if len(states) == 4:
            latent, mask = states[2], states[3]
        elif len(states) == 3:
            if self.has_latent:
                latent = states[2]
            else:
                mask = states[2]
        tail = tuple(torch.zeros_like(s) for s in states[2:])
        if self.divergence == 'none':
            # cnf.py:82-84 returns a tuple one element short of the state; here the log-det share is an explicit zero
            return (self.diffeq(t, y, latent=latent, mask=mask), torch.zeros_like(y)) + tail
        if self.divergence == 'exact':
            dy, div = self.diffeq(t, y, latent=latent, mask=mask)
            return (dy, -div) + tail
        if self._e is None and self.divergence == 'approximate':          # (drawn in eval mode too, where it is not used)
            if self.rademacher:
                self._e = torch.randint(low=0, high=2, size=y.shape).to(y) * 2 - 1          # cnf.py:76-80
            else:
                self._e = torch.randn_like(y)
        with torch.enable_grad():
            if not y.requires_grad:
                y = y.detach().requires_grad_(True)
            dy = self.diffeq(t, y, latent=latent, mask=mask)
            if not self.training or 'compute' in self.divergence:
                if self.set_data or self.divergence == 'compute_set':
                    div = divergence_exact_for_sets(dy, y)
                else:
                    div = divergence_exact(dy, y)
            else:
                div = divergence_approx(dy, y, self._e)
        return (dy, -div) + tail


def _rk_step(func, solver: str, t, t_next, y):
    """One step of the fixed-grid family on a tuple state: -> the increments.  Scalars t, t_next are fp32 numpy scalars, so stage
    times are fp32; the operation order is the kernel's (and the fixture solver's)."""
    f32 = np.float32
    dt = t_next - t
    h = float(dt)                       # (tensor * python float: the fp32 value, exactly)
    k1 = func(t, y)
    if solver == 'euler':
        return tuple(k * h for k in k1)
    if solver == 'midpoint':
        half = f32(0.5) * dt
        k2 = func(t + half, tuple(a + k * float(half) for a, k in zip(y, k1)))
        return tuple(k * h for k in k2)
    third, two_thirds = f32(1.0 / 3.0), f32(2.0 / 3.0)
    th = float(third)
    k2 = func(t + dt * third, tuple(a + (k * h) * th for a, k in zip(y, k1)))
    k3 = func(t + dt * two_thirds, tuple(a + (b - k * th) * h for a, k, b in zip(y, k1, k2)))
    k4 = func(t_next, tuple(a + ((k - b) + c) * h for a, k, b, c in zip(y, k1, k2, k3)))
    return tuple((((k + (b + c) * 3.0) + d) * h) * 0.125 for k, b, c, d in zip(k1, k2, k3, k4))


class _Tier(NamedTuple):
    """One inference kernel in ContinuousTransform's order of preference."""
    entry: str                 # the library's entry point
    applies: Callable          # (ODEfunc, x.dim()) -> does this setting ask for what the kernel computes?
    plan: Callable             # (transform, x.shape, latent_dim, trace, device) -> (net descriptor, keep-alive list) | None


def _set_setting(func, nd: int) -> bool:
    """Sets (..., N, dim) under no divergence or the exact divergence of a set net."""
    return nd >= 2 and (func.divergence == 'none' or func.exact_set_trace())


class ContinuousTransform(Transform):
    """Continuous normalizing flow dx/dt = net(t, x, latent) from 0 to T (cnf.py:102-262).

    >>> f = stribor_amd.ContinuousTransform(dim, net=stribor_amd.net.DiffeqMLP(dim + 1, [64], dim), solver='rk4',
    ...                                      solver_options={'step_size': 0.05})

    solver: 'euler', 'midpoint' or 'rk4' run (fixed grid; ``solver_options={'step_size': h}``, else the single step [0, T]).  The
    reference's default 'dopri5' and the other adaptive / Adams names construct and load but raise ``NotImplementedError`` when
    evaluated: pass ``solver='rk4', solver_options={'step_size': ...}``, or ``solver='dopri5_per_sample'`` for error control to
    ``atol`` / ``rtol`` per sample (``solver_options``: ``first_step``, else chosen per sample; ``max_num_steps``, default 4096 attempts
    per sample, after which the sample returns NaN with status 1 in ``last_solver_stats``).  ``use_adjoint`` is recorded and does not change the
    arithmetic: gradients are those of ``odeint`` through the discretised steps (``odeint_adjoint``'s differ from them by
    discretisation error only).  ``atol`` / ``rtol`` steer 'dopri5_per_sample'; a fixed grid does not use them."""

    def __init__(self, dim: int, net: nn.Module = None, T: float = 1.0, divergence: str = 'approximate', use_adjoint: bool = True,
                 has_latent: bool = False, solver: str = 'dopri5', solver_options: Optional[Dict] = {}, test_solver: str = None,
                 test_solver_options: Optional[Dict] = None, set_data: bool = False, rademacher: bool = False, atol: float = 1e-5,
                 rtol: float = 1e-3, **kwargs):
        super().__init__()
        self.T = T
        self.dim = dim
        self.odefunc = ODEfunc(net, divergence, rademacher, has_latent, set_data)
        self.use_adjoint = use_adjoint
        self.solver = solver
        self.solver_options = solver_options
        self.test_solver = test_solver or solver
        self.test_solver_options = solver_options if test_solver_options is None else test_solver_options
        self.atol = atol
        self.rtol = rtol
        self._trace = ProgramCache()
        self._last_path = None             # 'kernel' | 'composed': which path the last call took (tests, tools/bench_cnf.py)
        self.last_solver_stats = None      # an adaptive solve's int32 [..., 3] per sample: accepted steps, rejected steps, status

    # ---- the grid ---------------------------------------------------------------------------------------------------------------
    def _solver_name(self):
        return self.solver if self.training else self.test_solver

    def _solver(self):
        name = self._solver_name()
        opts = self.solver_options if self.training else self.test_solver_options
        if name in ADAPTIVE_SOLVERS:
            self._adaptive_options()
            return name, None
        if name not in FIXED_SOLVERS:
            raise NotImplementedError(
                f'stribor_amd: solver {name!r} is not implemented; the implemented solvers are {", ".join(FIXED_SOLVERS)} on a fixed '
                f"grid -- e.g. solver='rk4', solver_options={{'step_size': 0.05}} -- and {', '.join(ADAPTIVE_SOLVERS)} with atol / rtol")
        opts = dict(opts or {})
        step = opts.pop('step_size', None)
        if opts:
            raise NotImplementedError(f'stribor_amd: solver options {sorted(opts)} are not implemented (step_size only)')
        return name, (None if step is None else float(step))

    def _adaptive_options(self):
        """(first_step | None: automatic, max_num_steps) of an adaptive solve; any other option raises."""
        opts = dict((self.solver_options if self.training else self.test_solver_options) or {})
        first, cap = opts.pop('first_step', None), opts.pop('max_num_steps', MAX_NUM_STEPS)
        if opts:
            raise NotImplementedError(f'stribor_amd: solver options {sorted(opts)} are not implemented (first_step and max_num_steps only)')
        if first is not None and not float(first) > 0:
            raise ValueError(f'first_step must be positive (got {first})')
        if not 1 <= int(cap) <= _hip.CNF_ADAPTIVE_MAX_STEPS:
            raise ValueError(f'max_num_steps must be in 1..{_hip.CNF_ADAPTIVE_MAX_STEPS} (got {cap})')
        return (None if first is None else float(first)), int(cap)

    def _grid(self, reverse: bool):
        name, step = self._solver()
        if name in ADAPTIVE_SOLVERS:
            raise ValueError(f'stribor_amd: solver {name!r} has no fixed grid')
        t0, t1 = (self.T, 0.0) if reverse else (0.0, self.T)
        return Grid(name, step, fixed_grid(t0, t1, step))

    # ---- the kernel plans: (net descriptor, keep-alive list), or None outside the kernel's coverage -----------------------------
    def _kernel_net(self, latent_dim: int, want_ldj: bool, device):
        """(sx_cnf_net, keep-alive list [W1, b1, W2, b2, ...(, trace constants)]) for sx_cnf_flow, or None when the ODE function is
        outside its coverage."""
        diffeq = self.odefunc.diffeq
        if type(diffeq) is not DiffeqMLP or type(diffeq.net) is not MLP:
            return None
        mlp = diffeq.net
        lins = cover.linear_stack(mlp.net)
        if mlp._wrapped or mlp.final_activation_name is not None or lins is None or len(lins) not in (2, 3):
            return None
        # (MLP also takes an activation instance)
        if not cover.kernel_activation(mlp.activation_name, list(mlp.net)[1::2]):
            return None
        if not 1 <= self.dim <= _hip.CNF_MAX_DIM or lins[0].in_features != 1 + self.dim + latent_dim or lins[0].in_features > 128:
            return None
        if lins[-1].out_features != self.dim or any(l.out_features > 128 for l in lins[:-1]):
            return None
        keep = [p for lin in lins for p in (lin.weight, lin.bias)]
        if not cover.kernel_tensors([p for p in keep if p is not None], device):
            return None
        d = _hip.sx_cnf_net()
        for i, lin in enumerate(lins):
            d.layer[i].W, d.layer[i].b = lin.weight.data_ptr(), (0 if lin.bias is None else lin.bias.data_ptr())
            d.layer[i].out_dim, d.layer[i].in_dim = lin.weight.shape
        d.n_layers, d.dim, d.latent_dim, d.act = len(lins), self.dim, latent_dim, _hip.ACT_CODES[mlp.activation_name]
        if want_ldj:
            tc = self._trace_constants([l.weight for l in lins], device)
            keep.append(tc)
            d.trace = tc.data_ptr()
        lds = _hip.lib().sx_cnf_lds_bytes(d, int(want_ldj))
        if lds == 0 or lds > _hip.CNF_LDS_BYTES:
            return None
        return d, keep

    def _train_kernel_net(self, latent_dim: int, device):
        """(sx_cnf_net, keep-alive list [W1, b1, W2, b2, ...]) for sx_cnf_train_fwd / sx_cnf_train_bwd, or None outside their coverage
        (DESIGN.md "CNF": dim <= 32, 1 + dim + latent <= 64, hidden layers of <= 32 units)."""
        plan = self._kernel_net(latent_dim, False, device)
        if plan is None or _hip.lib().sx_cnf_train_lds_bytes(plan[0], 1) == 0 or _hip.lib().sx_cnf_train_lds_bytes(plan[0], 0) == 0:
            return None
        return plan

    def _adaptive_kernel_net(self, latent_dim: int, want_trace: bool, device):
        """(sx_cnf_net, keep-alive list) for sx_cnf_adaptive_flow, or None outside its coverage (dim <= 32, 1 + dim + latent <= 128,
        hidden layers of <= 64 units)."""
        plan = self._kernel_net(latent_dim, want_trace, device)
        if plan is None or _hip.lib().sx_cnf_adaptive_lds_bytes(plan[0]) == 0:
            return None
        return plan

    def _train_forward(self, x2, lat2, e2, name, step, grid, ckpt=None):
        """sx_cnf_train_fwd on rows -> (y, ldj [n]); `ckpt` [n_steps, n, dim] receives the state at the start of every step."""
        d, keep = self._train_kernel_net(0 if lat2 is None else lat2.shape[-1], x2.device)
        n = x2.shape[0]
        y = torch.empty_like(x2)
        ldj = torch.empty(n, dtype=torch.float32, device=x2.device)
        if n:
            _hip.call('sx_cnf_train_fwd', x2, ctypes.byref(d), x2.data_ptr(), _hip.ptr(lat2), e2.data_ptr(), y.data_ptr(), ldj.data_ptr(),
                      _hip.ptr(ckpt), *Grid(name, step, grid).c_args(n))
        del keep
        return y, ldj

    def _draw_noise(self, x):
        """The Hutchinson noise of one solve, drawn as the composition path's first evaluation draws it (cnf.py:76-80) and left in
        odefunc._e."""
        func = self.odefunc
        func.before_odeint()
        if func.rademacher:
            func._e = torch.randint(low=0, high=2, size=x.shape).to(x) * 2 - 1
        else:
            func._e = torch.randn_like(x)
        return func._e

    def _trace_constants(self, weights, device):
        """c / C of `trace_constants` as the kernel reads them: fp32 on the device, C zero-padded to a square of whole tiles.
        Derived in fp64 with batched torch ops; cached until a weight changes (ProgramCache: (data_ptr, _version) guards and the
        structure epoch)."""
        def build():
            with torch.no_grad():
                tc = trace_constants([w.detach().to(torch.float64) for w in weights], self.dim)
                if tc.dim() == 2:
                    P = 32 * max(cover.tiles(tc.shape[0]), cover.tiles(tc.shape[1]))
                    full = torch.zeros(P, P, dtype=torch.float64, device=device)
                    full[:tc.shape[0], :tc.shape[1]] = tc
                    tc = full
                return tc.to(torch.float32).contiguous()
        return self._trace.get(('trace', str(device)), build, guards=list(weights))

    def _set_kernel_net(self, set_size: int, latent_dim: int, device):
        """(sx_cnf_set_net, keep-alive list) for sx_cnf_set_flow over sets of `set_size` elements, or None outside its coverage."""
        diffeq = self.odefunc.diffeq
        if type(diffeq) is not DiffeqDeepset or type(diffeq.net) is not EquivariantNet:
            return None
        net = diffeq.net
        act = type(net.activation).__name__
        if type(net.final_activation) is not nn.Identity or not cover.kernel_activation(act, [net.activation]):
            return None
        layers = list(net.layers)
        if len(layers) not in (2, 3) or any(type(l) is not EquivariantLayer or type(l.l1) is not nn.Linear or type(l.l2) is not nn.Linear
                                            for l in layers):
            return None
        if not 1 <= set_size <= _hip.CNF_SET_MAX_SIZE or not 1 <= self.dim <= _hip.CNF_SET_MAX_DIM:
            return None
        widths = [1 + self.dim + latent_dim] + [l.l1.out_features for l in layers]
        if widths[0] > _hip.CNF_SET_MAX_IN or widths[-1] != self.dim or any(w > _hip.CNF_SET_MAX_HIDDEN for w in widths[1:-1]):
            return None
        if any(l.l1.in_features != w or l.l2.in_features != w or l.l2.out_features != l.l1.out_features for l, w in zip(layers, widths)):
            return None
        tensors = [t for l in layers for t in (l.l1.weight, l.l2.weight, l.l1.bias, l.l2.bias)]
        if not cover.kernel_tensors(tensors, device):
            return None
        image, offsets = self._set_constants(layers, set_size, device)
        d = _hip.sx_cnf_set_net()
        base = image.data_ptr()
        for i, l in enumerate(layers):
            d.A[i], d.G[i], d.bias[i] = l.l1.weight.data_ptr(), base + 4 * offsets[f'G{i}'], base + 4 * offsets[f'b{i}']
            d.out_dim[i] = l.l1.out_features
        d.w0, d.trace = base + 4 * offsets['w0'], base + 4 * offsets['trace']
        d.n_layers, d.dim, d.latent_dim, d.act, d.set_size = len(layers), self.dim, latent_dim, _hip.ACT_CODES[act], set_size
        if _hip.lib().sx_cnf_set_lds_bytes(d, 1) == 0:
            return None
        return d, [image] + [t.detach() for t in tensors]

    def _set_constants(self, layers, set_size: int, device):
        """What sx_cnf_set_flow reads beside the l1 weights, as one fp32 device buffer and float offsets into it: per layer G = l2.weight
        / N and bias = l1.bias + l2.bias / N, the time column w0 and `set_trace_constants` (two hidden layers: zero-padded to squares of
        whole tiles).  Derived in fp64; cached per N until a weight changes (ProgramCache guards and the structure epoch)."""
        guards = [t for l in layers for t in (l.l1.weight, l.l2.weight, l.l1.bias, l.l2.bias)]

        def build():
            with torch.no_grad():
                f64 = lambda t: t.detach().to(torch.float64)
                parts = {}
                for i, l in enumerate(layers):
                    parts[f'G{i}'] = f64(l.l2.weight) / set_size
                    parts[f'b{i}'] = f64(l.l1.bias) + f64(l.l2.bias) / set_size
                parts['w0'] = f64(layers[0].l1.weight)[:, 0] + f64(layers[0].l2.weight)[:, 0]
                tc = set_trace_constants([(f64(l.l1.weight), f64(l.l2.weight)) for l in layers], self.dim, set_size)
                if tc.dim() == 3:
                    P = 32 * max(cover.tiles(tc.shape[1]), cover.tiles(tc.shape[2]))
                    full = torch.zeros(5, P, P, dtype=torch.float64, device=device)
                    full[:, :tc.shape[1], :tc.shape[2]] = tc
                    tc = full
                parts['trace'] = tc
                offsets, off = {}, 0
                for k, v in parts.items():
                    offsets[k] = off
                    off += (v.numel() + 3) // 4 * 4                   # (every part 16-byte aligned)
                image = torch.zeros(off, dtype=torch.float32, device=device)
                for k, v in parts.items():
                    image[offsets[k]:offsets[k] + v.numel()] = v.reshape(-1).to(torch.float32)
                return image, offsets
        return self._trace.get(('set', set_size, str(device)), build, guards=guards)

    def _attn_kernel_net(self, set_size: int, latent_dim: int, device):
        """(sx_cnf_attn_net, keep-alive list) for sx_cnf_attn_flow over sets of `set_size` elements, or None outside its coverage.  The
        kernel reads the module's own parameters: there is no derived constant to cache."""
        diffeq = self.odefunc.diffeq
        if type(diffeq) is not DiffeqSelfAttention or type(diffeq.net) is not SelfAttention:
            return None
        net = diffeq.net
        embeds = (net.query, net.key, net.value)
        if any(type(m) is not MLP or m._wrapped or m.final_activation_name is not None for m in embeds):
            return None
        act = embeds[0].activation_name
        lins = [cover.linear_stack(m.net) for m in embeds]
        if lins[0] is None or len(lins[0]) not in (1, 2) or any(l is None or len(l) != len(lins[0]) for l in lins):
            return None
        n_hidden = len(lins[0]) - 1
        # (one activation, the same in the three embeddings)
        if n_hidden and not all(m.activation_name == act and cover.kernel_activation(act, [m.net[1]]) for m in embeds):
            return None
        proj = net.proj
        if not isinstance(proj, nn.Linear):
            return None
        E, in_dim = lins[0][-1].out_features, 1 + self.dim + latent_dim
        H1 = lins[0][0].out_features
        if any(l[0].in_features != in_dim or l[0].out_features != H1 or l[-1].out_features != E or l[-1].in_features != (H1 if n_hidden else in_dim)
               for l in lins) or proj.in_features != E or proj.out_features != self.dim:
            return None
        tensors = [t for l in lins for lin in l for t in (lin.weight, lin.bias)] + [proj.weight, proj.bias]
        if not cover.kernel_tensors(tensors, device):
            return None
        d = _hip.sx_cnf_attn_net()
        for i, l in enumerate(lins):
            d.W1[i], d.b1[i] = l[0].weight.data_ptr(), l[0].bias.data_ptr()
            if n_hidden:
                d.W2[i], d.b2[i] = l[1].weight.data_ptr(), l[1].bias.data_ptr()
        d.P, d.pb = proj.weight.data_ptr(), proj.bias.data_ptr()
        d.dim, d.latent_dim, d.act, d.set_size = self.dim, latent_dim, (_hip.ACT_CODES[act] if n_hidden else 0), set_size
        d.n_hidden, d.embed, d.n_heads, d.mask_diagonal = n_hidden, E, int(net.n_heads), int(bool(net.mask_diagonal))
        d.hidden[0] = H1 if n_hidden else 0
        if _hip.lib().sx_cnf_attn_lds_bytes(d) == 0:
            return None
        return d, [t.detach() for t in tensors]

    # per kind of exact-trace kernel: (guards, image builder, descriptor, LDS size entry, floats of LDS behind the image, the net's own
    # field <- the structure dict's key); the kind is also the cache key
    _EXACT_KINDS = {
        'exact': (exact_trace.kernel_tensors, exact_trace.kernel_image, 'sx_cnf_exact_net', 'sx_cnf_exact_lds_bytes', 0, None),
        'exact_set': (exact_trace.kernel_tensors_set, exact_trace.kernel_image_set, 'sx_cnf_exact_set_net', 'sx_cnf_exact_set_lds_bytes',
                      exact_trace.SET_EXCHANGE_FLOATS, ('pooling', lambda s: exact_trace.POOLINGS[s['pooling']])),
        'exact_attn': (exact_trace.kernel_tensors_attn, exact_trace.kernel_image_attn, 'sx_cnf_exact_attn_net', 'sx_cnf_exact_attn_lds_bytes',
                       exact_trace.ATTN_EXCHANGE_FLOATS, ('n_heads', lambda s: s['heads'])),
    }

    def _exact_plan(self, s, latent_dim: int, device, kind: str = 'exact', set_size=None):
        """(net descriptor, keep-alive list) of an exact-trace structure dict `s` (exact_trace.kernel_coverage / kernel_coverage_set /
        kernel_coverage_attn; None: not covered) for the kernel of `kind` ('exact': sx_cnf_exact_flow; 'exact_set' / 'exact_attn', with a
        `set_size`: sx_cnf_exact_set_flow / sx_cnf_exact_attn_flow), or None outside the kernel's coverage."""
        if s is None:
            return None
        tensors, build_image, desc, lds_entry, behind, own = self._EXACT_KINDS[kind]
        guards = tensors(s)
        if not cover.kernel_tensors(guards, device):
            return None

        def build():
            image, w_latent = build_image(s)
            image = torch.from_numpy(image).to(device)
            return image, (None if w_latent is None else torch.from_numpy(w_latent).contiguous().to(device))
        image, w_latent = self._trace.get((kind, str(device)), build, guards=guards)
        d = getattr(_hip, desc)()
        d.image, d.w_latent, d.image_floats = image.data_ptr(), (0 if w_latent is None else w_latent.data_ptr()), image.numel()
        d.dim, d.d_h, d.latent_dim, d.n_hidden, d.act = self.dim, s['d_h'], latent_dim, len(s['hidden']), _hip.ACT_CODES[s['act']]
        for i, w in enumerate(s['hidden']):
            d.hidden[i] = w
        if own is not None:
            d.set_size = set_size
            setattr(d, own[0], own[1](s))
        lds = getattr(_hip.lib(), lds_entry)(d)
        if lds == 0 or lds > _hip.CNF_LDS_BYTES or lds != 4 * (image.numel() + behind):
            return None
        return d, [image, w_latent]

    def _exact_kernel_net(self, latent_dim: int, device):
        """(sx_cnf_exact_net, keep-alive list) for sx_cnf_exact_flow, or None when the ODE function is outside its coverage."""
        return self._exact_plan(exact_trace.kernel_coverage(self.odefunc.diffeq, self.dim, latent_dim), latent_dim, device)

    def _exact_set_kernel_net(self, set_size: int, latent_dim: int, device):
        """(sx_cnf_exact_set_net, keep-alive list) for sx_cnf_exact_set_flow over sets of `set_size` elements, or None when the ODE
        function is outside its coverage."""
        s = exact_trace.kernel_coverage_set(self.odefunc.diffeq, self.dim, latent_dim, set_size)
        return self._exact_plan(s, latent_dim, device, 'exact_set', set_size)

    def _exact_attn_kernel_net(self, set_size: int, latent_dim: int, device):
        """(sx_cnf_exact_attn_net, keep-alive list) for sx_cnf_exact_attn_flow over sets of `set_size` elements, or None when the ODE
        function is outside its coverage."""
        s = exact_trace.kernel_coverage_attn(self.odefunc.diffeq, self.dim, latent_dim, set_size)
        return self._exact_plan(s, latent_dim, device, 'exact_attn', set_size)

    # ---- the two paths ----------------------------------------------------------------------------------------------------------
    def _solve_kernel(self, entry, plan, x2, lat2, grid, want_ldj):
        """One launch of an inference tier's entry point on rows -> (y, ldj [n] | None without `want_ldj`)."""
        d, keep = plan
        n = x2.shape[0]
        y = torch.empty_like(x2)
        ldj = torch.empty(n, dtype=torch.float32, device=x2.device) if want_ldj else None
        if n:
            _hip.call(entry, x2, ctypes.byref(d), x2.data_ptr(), _hip.ptr(lat2), y.data_ptr(), _hip.ptr(ldj), *grid.c_args(n), int(want_ldj))
        del keep
        return y, ldj

    def _solve_composed(self, x, latent, mask, name, grid, keep_graph: bool):
        """The same grid and tableau as torch ops over the module, on any leading shape -> (y, log-det [..., 1])."""
        func = self.odefunc
        func.before_odeint()
        state = (x, torch.zeros_like(x))
        if latent is not None:
            state += (latent,)
        if mask is not None:
            state += (mask,)
        for i in range(len(grid) - 1):
            inc = _rk_step(func, name, grid[i], grid[i + 1], state)
            state = tuple(a + b for a, b in zip(state[:2], inc[:2])) + state[2:]
            if not keep_graph:
                state = tuple(s.detach() for s in state)
        return state[0], -state[1].sum(-1, keepdim=True)

    def _composed_reference(self, x, latent=None, mask=None, reverse: bool = False):
        """The composition path without a graph (tests and tools/bench_cnf.py compare the kernel with it)."""
        if self._solver_name() in ADAPTIVE_SOLVERS:
            with torch.no_grad():
                return self._solve_composed_adaptive(x.to(torch.float32), latent, mask, reverse, False)[:2]
        name, step, grid = self._grid(reverse)
        with torch.no_grad():
            return self._solve_composed(x.to(torch.float32), latent, mask, name, grid, False)

    # ---- how a call picks its kernel --------------------------------------------------------------------------------------------
    # The inference tiers in order of preference: the first whose setting holds and whose planner returns a plan runs.  Exact-trace sets
    # (pooled, then attention) come before exact-trace because the set types are the narrower match; sets come before attention because the two planners key on
    # disjoint module types.  `applies` sees the ODEfunc and x.dim(); `plan` the transform, x.shape, the latent width, whether the kernel
    # accumulates the log-det, and the device.
    _TIERS = (
        _Tier('sx_cnf_flow', lambda func, nd: func.divergence == 'none' or func.exact_trace(),
              lambda f, shape, ld, trace, dev: f._kernel_net(ld, trace, dev)),
        # (the choice does not depend on set_data: ODEfunc ignores it under 'exact')
        _Tier('sx_cnf_exact_set_flow',
              lambda func, nd: func.divergence == 'exact' and nd >= 2 and type(func.diffeq) is exact_trace.DiffeqExactTraceDeepSet,
              lambda f, shape, ld, trace, dev: f._exact_set_kernel_net(shape[-2], ld, dev)),
        _Tier('sx_cnf_exact_attn_flow',
              lambda func, nd: func.divergence == 'exact' and nd >= 2 and type(func.diffeq) is exact_trace.DiffeqExactTraceAttention,
              lambda f, shape, ld, trace, dev: f._exact_attn_kernel_net(shape[-2], ld, dev)),
        _Tier('sx_cnf_exact_flow', lambda func, nd: func.divergence == 'exact' and not func.set_data,
              lambda f, shape, ld, trace, dev: f._exact_kernel_net(ld, dev)),
        _Tier('sx_cnf_set_flow', _set_setting, lambda f, shape, ld, trace, dev: f._set_kernel_net(shape[-2], ld, dev)),
        _Tier('sx_cnf_attn_flow', _set_setting, lambda f, shape, ld, trace, dev: f._attn_kernel_net(shape[-2], ld, dev)),
    )

    def _choose(self, shape, latent_dim: int, masked: bool, graph: bool, want_ldj: bool, device):
        """What runs a call on x of `shape` -> (route, plan, trace).  route: 'train' (the Hutchinson pair, asked first: it also serves
        calls that want a graph), a tier's entry point (no graph), or 'composed' (plan None; every masked call).  Under an adaptive
        solver: 'sx_cnf_adaptive_flow' where a fixed one would get 'sx_cnf_flow' and the adaptive planner covers the net, else 'composed'
        -- sets, masks, calls that want a graph, training mode and the other five tiers' nets are all composed for now.  trace: does the kernel
        accumulate the log-det.  Host code only: `device` may be the CPU."""
        func = self.odefunc
        trace = want_ldj and func.divergence != 'none'
        if masked:
            return 'composed', None, trace
        if self._solver_name() in ADAPTIVE_SOLVERS:
            # the dense tier's setting and no graph, or composed; the kernel integrates the trace whenever there is one (it is part of
            # the error norm), whether or not the caller takes the log-det
            if not graph and self._TIERS[0].applies(func, len(shape)):
                plan = self._adaptive_kernel_net(latent_dim, func.divergence != 'none', device)
                if plan is not None:
                    return 'sx_cnf_adaptive_flow', plan, trace
            return 'composed', None, trace
        if func.divergence == 'approximate' and self.training and not func.set_data:
            plan = self._train_kernel_net(latent_dim, device)
            if plan is not None:
                return 'train', plan, trace
        if not graph:
            for tier in self._TIERS:
                plan = tier.plan(self, shape, latent_dim, trace, device) if tier.applies(func, len(shape)) else None
                if plan is not None:
                    return tier.entry, plan, trace
        return 'composed', None, trace

    def _solve(self, x, latent, mask, reverse: bool, want_ldj: bool):
        _hip.require_device(x, 'x')
        if self._solver_name() in ADAPTIVE_SOLVERS:
            return self._solve_adaptive(x, latent, mask, reverse, want_ldj)
        grid = self._grid(reverse)
        out_dtype = x.dtype
        x = x.to(torch.float32)
        latent_dim = 0 if latent is None else latent.shape[-1]
        if latent is not None:
            latent = latent.to(device=x.device, dtype=torch.float32).expand(*x.shape[:-1], latent_dim)
        graph = graph_wanted(self, x, latent)
        route, plan, trace = self._choose(x.shape, latent_dim, mask is not None, graph, want_ldj, x.device)
        if route == 'composed':
            with torch.set_grad_enabled(graph):
                y, ldj = self._solve_composed(x, latent, mask, grid.name, grid.points, graph)
        else:
            x2, lead = flatten_rows(x)
            lat2 = None if latent is None else flatten_rows(latent)[0]
            if route != 'train':
                with torch.no_grad():
                    y2, ldj = self._solve_kernel(route, plan, x2, lat2, grid, trace)
            else:
                # training with the Hutchinson estimator: one forward launch (with checkpoints when a graph is wanted) and one adjoint
                e2 = flatten_rows(self._draw_noise(x))[0]
                if graph:
                    y2, ldj = _CNFTrain.apply(self, *grid, x2, lat2, e2, *plan[1])         # (the keep-alive list: W1, b1, W2, b2, ...)
                else:
                    with torch.no_grad():
                        y2, ldj = self._train_forward(x2, lat2, e2, *grid)
            if not want_ldj:
                ldj = None
            elif ldj is None:                                           # (divergence 'none')
                ldj = torch.zeros(x2.shape[0], dtype=torch.float32, device=x.device)
            y, ldj = y2.reshape(*lead, self.dim), (None if ldj is None else ldj.reshape(*lead, 1))
        self._last_path = 'composed' if route == 'composed' else 'kernel'
        self.odefunc._num_evals.fill_((len(grid.points) - 1) * STAGES[grid.name])
        return (y.to(out_dtype) if out_dtype == torch.bfloat16 else y), ldj

    # ---- the per-sample adaptive solver ('dopri5_per_sample', DESIGN.md "CNF") ---------------------------------------------------
    def _solve_adaptive(self, x, latent, mask, reverse: bool, want_ldj: bool):
        first_step, max_steps = self._adaptive_options()
        out_dtype = x.dtype
        x = x.to(torch.float32)
        latent_dim = 0 if latent is None else latent.shape[-1]
        if latent is not None:
            latent = latent.to(device=x.device, dtype=torch.float32).expand(*x.shape[:-1], latent_dim)
        graph = graph_wanted(self, x, latent)
        route, plan, trace = self._choose(x.shape, latent_dim, mask is not None, graph, want_ldj, x.device)
        if route == 'composed':
            with torch.set_grad_enabled(graph):
                y, ldj, stats = self._solve_composed_adaptive(x, latent, mask, reverse, graph)
        else:
            x2, lead = flatten_rows(x)
            lat2 = None if latent is None else flatten_rows(latent)[0]
            d, keep = plan
            n = x2.shape[0]
            want_trace = self.odefunc.divergence != 'none'
            t0, t1 = (self.T, 0.0) if reverse else (0.0, self.T)
            with torch.no_grad():
                y2 = torch.empty_like(x2)
                l2 = torch.empty(n, dtype=torch.float32, device=x.device) if want_trace else None
                stats = torch.empty(n, 3, dtype=torch.int32, device=x.device)
                if n:
                    _hip.call(route, x2, ctypes.byref(d), x2.data_ptr(), _hip.ptr(lat2), y2.data_ptr(), _hip.ptr(l2), stats.data_ptr(), n,
                              float(t0), float(t1), float(self.rtol), float(self.atol), float(first_step or 0.0), max_steps, int(want_trace))
            del keep
            if not want_ldj:
                l2 = None
            elif l2 is None:                                            # (divergence 'none')
                l2 = torch.zeros(n, dtype=torch.float32, device=x.device)
            y, ldj, stats = y2.reshape(*lead, self.dim), (None if l2 is None else l2.reshape(*lead, 1)), stats.reshape(*lead, 3)
        self._last_path = 'composed' if route == 'composed' else 'kernel'
        self.last_solver_stats = stats
        # evaluations of the slowest sample, left on the device: reading it (_num_evals) synchronises, the solve does not
        with torch.no_grad():
            steps = stats[..., :2].sum(-1).max() if stats.numel() else torch.zeros((), dtype=torch.int32, device=x.device)
            self.odefunc._num_evals.copy_(steps * 6 + (1 if first_step is not None else 2))
        return (y.to(out_dtype) if out_dtype == torch.bfloat16 else y), ldj

    def _solve_composed_adaptive(self, x, latent, mask, reverse: bool, keep_graph: bool):
        """The controller of sx_cnf_adaptive_flow as vectorised torch ops over the module, one step size per sample, on any leading
        shape, mask and net whose time argument may be a tensor (every DiffeqConcat) -> (y, log-det [..., 1], stats [samples, 3]).  A
        sample is a row, or under `set_data` a set.  Accepting is a `torch.where`; with `keep_graph` the step sizes and the accept
        decisions are constants and the graph runs through the accepted arithmetic (discretise-then-optimise with frozen steps)."""
        func = self.odefunc
        if func.divergence == 'exact':
            raise NotImplementedError("stribor_amd: the exact-trace nets take one time for the whole batch; 'dopri5_per_sample' needs one per sample")
        func.before_odeint()
        first_step, max_steps = self._adaptive_options()
        rtol, atol = float(self.rtol), float(self.atol)
        t0, t1 = (self.T, 0.0) if reverse else (0.0, self.T)
        sgn = -1.0 if t1 < t0 else 1.0
        T = float(abs(np.float32(t1) - np.float32(t0)))
        nsd = 2 if self.set_data and x.dim() >= 2 else 1                 # trailing axes of one sample
        lead = x.shape[:-nsd]
        want = func.divergence != 'none'
        tail = (() if latent is None else (latent,)) + (() if mask is None else (mask,))
        col = lambda v: v.reshape(*lead, *([1] * nsd))                  # a per-sample scalar against x ...
        row = lambda v: v.reshape(*lead, *([1] * (nsd - 1)))            # ... and against the trace integral a [..., (N)]
        rms = lambda v: v.reshape(*lead, -1).pow(2).mean(-1).sqrt()
        norm = lambda vx, va: torch.maximum(rms(vx), rms(va)) if want else rms(vx)
        tab = DOPRI5
        A = [[_r32(v) for v in r] for r in tab.a]
        C, E = [_r32(v) for v in tab.c], [_r32(v) for v in tab.e]

        def f(s, xs):                                                    # sgn f and sgn tr df/dx at t0 + sgn s
            out = func(col(s) * sgn + t0, (xs, torch.zeros_like(xs)) + tail)
            return out[0] * sgn, -out[1].sum(-1) * sgn

        def weighted(w, ks):                                            # sum_j w_j k_j, left to right, zero weights left out
            acc = None
            for wj, kj in zip(w, ks):
                if wj != 0.0:
                    acc = kj * wj if acc is None else acc + kj * wj
            return acc

        zeros = lambda dtype: torch.zeros(lead, dtype=dtype, device=x.device)
        y, a, s = x, torch.zeros(x.shape[:-1], dtype=torch.float32, device=x.device), zeros(torch.float32)
        k1, q1 = f(s, y)
        with torch.no_grad():
            if first_step is not None:
                dt = torch.full(lead, first_step, dtype=torch.float32, device=x.device)
            else:
                scale = atol + rtol * y.abs()
                d0, d1 = rms(y / scale), norm(k1 / scale, q1 / atol)
                h0 = torch.where((d0 < 1e-5) | (d1 < 1e-5), torch.full_like(d0, 1e-6), 0.01 * d0 / d1)
                kp, qp = f(h0, y + col(h0) * k1)
                d2 = norm((kp - k1) / scale, (qp - q1) / atol) / h0
                dm = torch.where((d1 > d2) | (d1 != d1), d1, d2)
                h1 = torch.where((d1 <= 1e-15) & (d2 <= 1e-15), torch.clamp(1e-3 * h0, min=1e-6), (0.01 / dm).pow(0.2))
                dt = torch.where((100.0 * h0 < h1) | (h0 != h0), 100.0 * h0, h1)
            done = zeros(torch.bool) | (not T > 0.0)
        n_att, n_acc, n_rej, status = (zeros(torch.int32) for _ in range(4))
        while True:
            with torch.no_grad():
                rem = T - s
                last = dt >= rem
                h = torch.where(last, rem, dt)
                cap = ~done & (n_att >= max_steps)
                status, done = torch.where(cap, 1, status), done | cap
                under = ~done & (s + h == s)
                status, done = torch.where(under, 2, status), done | under
                if bool(done.all()):
                    break
                act = ~done
                h = torch.where(act, h, torch.zeros_like(h))
                n_att = n_att + act
                hx, ha = col(h), row(h)
            K, Q = [k1], [q1]
            for st in range(1, 7):
                xs = y + hx * weighted(A[st], K)
                k, q = f(s + C[st] * h, xs)
                K.append(k)
                Q.append(q)
            a1 = a + ha * weighted(A[6], Q)                      # (xs is the step: a7 = b)
            with torch.no_grad():
                err_x, err_a = hx * weighted(E, K), ha * weighted(E, Q)
                tol_x = atol + rtol * torch.maximum(y.abs(), xs.abs())
                tol_a = atol + rtol * torch.maximum(a.abs(), a1.abs())
                ratio = norm(err_x / tol_x, err_a / tol_a)
                finite = torch.isfinite(ratio)
                accept = act & finite & (ratio <= 1.0)
                floor = torch.where(ratio < 1.0, 1.0, 0.2).to(ratio)
                factor = torch.where(ratio == 0.0, torch.full_like(ratio, 10.0), torch.clamp(torch.maximum(0.9 * ratio.pow(-0.2), floor), max=10.0))
                s = torch.where(accept, torch.where(last, torch.full_like(s, T), s + h), s)
                n_acc, n_rej = n_acc + accept, n_rej + (act & ~accept)
                bad = act & ~finite
                status, done = torch.where(bad, 2, status), done | bad | (accept & last)
                dt = torch.where(act, h * factor, dt)
            y, a = torch.where(col(accept), xs, y), torch.where(row(accept), a1, a)
            k1, q1 = torch.where(col(accept), K[6], k1), torch.where(row(accept), Q[6], q1)
            if not keep_graph:
                y, a, k1, q1 = y.detach(), a.detach(), k1.detach(), q1.detach()
        failed = status != 0
        nan = torch.full((), float('nan'), dtype=torch.float32, device=x.device)
        y, a = torch.where(col(failed), nan, y), torch.where(row(failed), nan, a)
        return y, a.unsqueeze(-1), torch.stack([n_acc, n_rej, status], -1).to(torch.int32)

    # ---- reference method set ---------------------------------------------------------------------------------------------------
    def forward_and_log_det_jacobian(self, x, latent=None, mask=None, *, reverse=False, **kwargs):
        return self._solve(x, latent, mask, bool(reverse), True)

    def inverse_and_log_det_jacobian(self, y, latent=None, mask=None, **kwargs):
        return self._solve(y, latent, mask, True, True)

    def forward(self, x, latent=None, mask=None, **kwargs):
        return self._solve(x, latent, mask, False, False)[0]

    def inverse(self, y, latent=None, mask=None, **kwargs):
        return self._solve(y, latent, mask, True, False)[0]

    def log_det_jacobian(self, x, y=None, mask=None, latent=None, **kwargs):
        return self._solve(x, latent, mask, False, True)[1]

    def _num_evals(self):
        return self.odefunc._num_evals.item()

    # ---- inside a NormalizingFlow that trains layer by layer ----------------------------------------------------------------
    def _autograd_supported(self) -> bool:
        return True

    def _autograd_forward(self, x2, lat2=None):
        y, ldj = self._solve(x2, lat2, None, False, True)
        return y, ldj.reshape(-1)

    def _autograd_inverse(self, y2, lat2=None, pre=None):
        x, ldj = self._solve(y2, lat2, None, True, True)
        return x, ldj.reshape(-1)

    @property
    def set_data(self) -> bool:
        """Does the ODE function read its input as sets (..., N, dim)?  (NormalizingFlow keeps the set axis for such layers.)"""
        return bool(self.odefunc.set_data or self.odefunc.divergence == 'compute_set'
                    or type(self.odefunc.diffeq) in (DiffeqZeroTraceDeepSet, exact_trace.DiffeqExactTraceDeepSet, DiffeqZeroTraceAttention,
                                                     exact_trace.DiffeqExactTraceAttention))

    def _autograd_set(self, x2, lat2, set_size: int, reverse: bool):
        lat = None if lat2 is None else lat2.reshape(-1, set_size, lat2.shape[-1])
        y, ldj = self._solve(x2.reshape(-1, set_size, x2.shape[-1]), lat, None, reverse, True)
        return y.reshape(x2.shape), ldj.reshape(-1)
