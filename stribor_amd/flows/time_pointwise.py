"""Time-dependent element-wise flows (reference: stribor/flows/activations.py:125-196): ``ContinuousActivation`` and ``ContinuousTanh``.
Both are the identity at ``t = 0``, which makes them ``NeuralFlow`` building blocks.  Same constructors and method sets; with one time
per row (any ``t`` that broadcasts to ``x.shape[:-1] + (1,)``) every call is one ``sx_pointwise_time`` launch (values, per-element
log-derivative and its row sum in the same pass), and inside a ``NeuralFlow`` each is one ``SX_STEP_POINTWISE_TIME`` step of the flow's
one-launch program.  Any other broadcastable ``t`` (a feature axis of width ``dim``), and a ``ContinuousActivation`` over a callable the
kernel does not cover, run the reference's lines as torch ops on the device.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _hip
from ..flow import ElementwiseTransform, flatten_rows, graph_rows, graph_wanted

__all__ = ['ContinuousActivation', 'ContinuousTanh']


def row_times(t, x):
    """One fp32 time per row of x[..., D] ([N], contiguous, differentiable in t), or None when t does not broadcast to
    x.shape[:-1] + (1,)."""
    lead = tuple(x.shape[:-1])
    if not torch.is_tensor(t):
        t = torch.as_tensor(t, dtype=torch.float32, device=x.device)
    try:
        if tuple(torch.broadcast_shapes(tuple(t.shape), lead + (1,))) != lead + (1,):
            return None
    except RuntimeError:
        return None
    return t.to(device=x.device, dtype=torch.float32).expand(*lead, 1).reshape(-1).contiguous()


def run_pointwise_time(x, t_rows, kind, param, want_y=True, want_ldj=False, want_ldiag=False):
    """Launch sx_pointwise_time on x[..., D] with one time per row -> (y | None, ldj[..., 1] | None, ldiag[..., D] | None)."""
    _hip.require_device(x, 'x')
    x2, lead = flatten_rows(x)
    n, d = x2.shape
    y = torch.empty_like(x2) if want_y else None
    ldj = torch.empty(n, dtype=torch.float32, device=x2.device) if want_ldj else None
    ldiag = torch.empty(n, d, dtype=torch.float32, device=x2.device) if want_ldiag else None
    _hip.call('sx_pointwise_time', x2, x2.data_ptr(), t_rows.data_ptr(), _hip.ptr(y), _hip.ptr(ldj), _hip.ptr(ldiag), n, d,
              _hip.dtype_code(x2), kind, float(param), 0)
    return (None if y is None else y.reshape(*lead, d), None if ldj is None else ldj.reshape(*lead, 1),
            None if ldiag is None else ldiag.reshape(*lead, d))


def _backward(x2, t_rows, gy, gldj, gldiag, kind, param, want_gt, want_gparam):
    """sx_pointwise_time_bwd -> (gx [N, D], gt [N] | None, gparam [] | None)."""
    n, d = x2.shape
    f32 = lambda g: None if g is None else g.to(torch.float32).contiguous()
    gy, gldj, gldiag = f32(gy), f32(gldj), f32(gldiag)
    if gy is None and gldj is None and gldiag is None:
        gy = torch.zeros_like(x2)
    gx = torch.empty_like(x2)
    gt = torch.empty(n, dtype=torch.float32, device=x2.device) if want_gt else None
    gparam = torch.empty(1, dtype=torch.float32, device=x2.device) if want_gparam else None
    partial = torch.empty(_hip.PWT_PARTIALS, dtype=torch.float64, device=x2.device) if want_gparam else None
    _hip.call('sx_pointwise_time_bwd', x2, x2.data_ptr(), t_rows.data_ptr(), _hip.ptr(gy), _hip.ptr(gldj), _hip.ptr(gldiag),
              gx.data_ptr(), _hip.ptr(gt), _hip.ptr(gparam), _hip.ptr(partial), n, d, kind, float(param))
    return gx, gt, (None if gparam is None else gparam.reshape(()))


class TanhFlowOp(torch.autograd.Function):
    """(y, row log-det[, per-element log-derivative]) of a tanh-flow kind as a differentiable op in x and the row times."""

    @staticmethod
    def forward(ctx, x2, t_rows, kind, log_time, want_ldiag=False):
        x2 = x2.contiguous()
        y, ldj, ldiag = run_pointwise_time(x2, t_rows, kind, float(log_time), want_ldj=True, want_ldiag=bool(want_ldiag))
        ctx.save_for_backward(x2, t_rows)
        ctx.meta = (kind, float(log_time))
        if want_ldiag:
            return y, ldj.reshape(-1), ldiag
        return y, ldj.reshape(-1)

    @staticmethod
    def backward(ctx, gy, gldj, gldiag=None):
        x2, t_rows = ctx.saved_tensors
        kind, log_time = ctx.meta
        gx, gt, _ = _backward(x2, t_rows, gy, gldj, gldiag, kind, log_time, ctx.needs_input_grad[1], False)
        return gx, gt, None, None, None


class TimeMixOp(torch.autograd.Function):
    """y of a mix kind as a differentiable op in x, the row times and the temperature (`temp`: its value on the host)."""

    @staticmethod
    def forward(ctx, x2, t_rows, temperature, kind, temp):
        x2 = x2.contiguous()
        y = run_pointwise_time(x2, t_rows, kind, temp)[0]
        ctx.save_for_backward(x2, t_rows)
        ctx.meta = (kind, temp)
        return y

    @staticmethod
    def backward(ctx, gy):
        x2, t_rows = ctx.saved_tensors
        kind, temp = ctx.meta
        gx, gt, gtemp = _backward(x2, t_rows, gy, None, None, kind, temp, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return gx, gt, gtemp, None, None


class ContinuousTanh(ElementwiseTransform):
    """activations.py:162-196: the solution of dx/dt = tanh x, y = asinh(exp(t) sinh x); ``log_time``: t -> log1p(t).  The kernel states
    it in the log domain: it stays finite where the reference's fp32 sequence overflows (|x| + t beyond ~89, its log-derivative ~44)."""

    def __init__(self, log_time: bool = False):
        super().__init__()
        self.log_time = log_time

    def _kind(self, reverse):
        return _hip.PWT_TANH_FLOW_INV if reverse else _hip.PWT_TANH_FLOW

    # ---- training inside a NormalizingFlow (layer-wise autograd path): the flow hands the call's `t` over by rows ------------------
    _autograd_takes_time = True

    def _autograd_supported(self) -> bool:
        return True

    def _autograd_forward(self, x2, lat2=None, t=None):
        return self._autograd_step(x2, t, False)

    def _autograd_inverse(self, x2, lat2=None, t=None):
        return self._autograd_step(x2, t, True)

    def _autograd_step(self, x2, t, reverse):
        """(rows, log-det [N]) of the direction's own map; t: [N, 1], [N, dim] (torch ops), a number or a 0-dim tensor."""
        if t is None:
            raise TypeError('ContinuousTanh needs a time `t`')                      # (the reference's forward has no default either)
        y, ldj, _ = self._run(x2, t, reverse, True, True, False)
        return y, ldj.reshape(-1)

    # ---- fused-program hook: one SX_STEP_POINTWISE_TIME step of a NeuralFlow program -------------------------------------------------
    def _plan_time(self, builder, reverse: bool, ldj_scale: float, time_sel: int) -> bool:
        builder.add_pointwise_time(self._kind(reverse), float(bool(self.log_time)), time_sel)
        return True

    # ---- torch ops for a t that is not one time per row: the reference's lines ---------------------------------------------------------
    def _torch_forward(self, x, t, reverse):
        _hip.require_device(x, 'x')
        t = torch.as_tensor(t, device=x.device)
        if self.log_time:
            t = torch.log1p(t)
        if reverse:
            t = -t
        return torch.asinh(t.exp() * torch.sinh(x))

    def _torch_log_diag(self, x, t, reverse=False):
        t = torch.as_tensor(t, device=x.device)
        if self.log_time:
            t = torch.log1p(t)
        if reverse:
            t = -t
        t = t.exp()
        return (t * torch.cosh(x) / torch.sqrt(torch.square(t * torch.sinh(x)) + 1)).log()

    def _run(self, x, t, reverse, want_y, want_ldj, want_ldiag):
        """(y | None, ldj [..., 1] | None, ldiag | None) of the direction's own map in one launch."""
        _hip.require_device(x, 'x')
        tr = row_times(t, x)
        if tr is None:
            ld = self._torch_log_diag(x, t, reverse) if (want_ldj or want_ldiag) else None
            return (self._torch_forward(x, t, reverse) if want_y else None, ld.sum(-1, keepdim=True) if want_ldj else None,
                    ld if want_ldiag else None)
        if graph_wanted(None, x, t):
            x2, _, lead = graph_rows(x)
            d = x2.shape[1]
            out = TanhFlowOp.apply(x2, tr, self._kind(reverse), self.log_time, want_ldiag)
            return out[0].reshape(*lead, d), out[1].reshape(*lead, 1), (out[2].reshape(*lead, d) if want_ldiag else None)
        return run_pointwise_time(x, tr, self._kind(reverse), float(bool(self.log_time)), want_y, want_ldj, want_ldiag)

    def forward(self, x, t, reverse: bool = False, **kwargs):
        return self._run(x, t, reverse, True, False, False)[0]

    def inverse(self, y, t, **kwargs):
        return self._run(y, t, True, True, False, False)[0]

    def log_diag_jacobian(self, x, y=None, t=None, **kwargs):
        return self._run(x, t, False, False, False, True)[2]

    def log_det_jacobian(self, x, y=None, t=None, **kwargs):
        return self._run(x, t, False, False, True, False)[1]

    def forward_and_log_det_jacobian(self, x, t, **kwargs):
        return self._run(x, t, False, True, True, False)[:2]

    def inverse_and_log_det_jacobian(self, y, t, **kwargs):
        return self._run(y, t, True, True, True, False)[:2]

    def forward_and_log_diag_jacobian(self, x, t, **kwargs):
        y, _, ld = self._run(x, t, False, True, False, True)
        return y, ld

    def inverse_and_log_diag_jacobian(self, y, t, **kwargs):
        x, _, ld = self._run(y, t, True, True, False, True)
        return x, ld


_MIX_FUNCTIONS = {torch.tanh: _hip.PWT_MIX_TANH, F.tanh: _hip.PWT_MIX_TANH, torch.sigmoid: _hip.PWT_MIX_SIGMOID,
                  F.sigmoid: _hip.PWT_MIX_SIGMOID, torch.relu: _hip.PWT_MIX_RELU, F.relu: _hip.PWT_MIX_RELU}
_MIX_MODULES = {nn.Tanh: _hip.PWT_MIX_TANH, nn.Sigmoid: _hip.PWT_MIX_SIGMOID, nn.ReLU: _hip.PWT_MIX_RELU}


class ContinuousActivation(ElementwiseTransform):
    """activations.py:125-159: x (1 - w) + activation(x) w with w = tanh(temperature t).  The kernel covers torch.tanh / torch.sigmoid /
    torch.relu, their torch.nn.functional twins and instances of exactly nn.Tanh / nn.Sigmoid / nn.ReLU; any other callable runs the
    reference's two lines as torch ops.  No inverse and no log-determinant, like the reference."""

    def __init__(self, activation, temperature: float = 1., learnable: bool = False):
        super().__init__()
        self.activation = activation
        self.temperature = nn.Parameter(torch.tensor(temperature), requires_grad=learnable)
        self._temp_seen = None

    def _kind(self):
        a = self.activation
        if isinstance(a, nn.Module):
            return _MIX_MODULES.get(type(a))
        try:
            return _MIX_FUNCTIONS.get(a)
        except TypeError:               # an unhashable callable
            return None

    def _temperature_value(self) -> float:
        """float(temperature), read back once per version of the parameter."""
        p = self.temperature
        key = (p.data_ptr(), p._version)
        if self._temp_seen is None or self._temp_seen[0] != key:
            self._temp_seen = (key, float(p.detach()))
        return self._temp_seen[1]

    def _autograd_supported(self) -> bool:
        """The layer-wise autograd path of a NormalizingFlow returns every layer's log-det, and this transform has none (the reference
        raises NotImplementedError): it does not join that path.  Its own forward is differentiable, and a NeuralFlow trains through it."""
        return False

    # ---- fused-program hook ----------------------------------------------------------------------------------------------------------
    def _plan_time(self, builder, reverse: bool, ldj_scale: float, time_sel: int) -> bool:
        kind = self._kind()
        if reverse or kind is None:
            return False
        builder.add_pointwise_time(kind, self._temperature_value(), time_sel)
        return True

    def _plan_guards(self) -> list:
        return [self.temperature]

    def forward(self, x, t, **kwargs):
        _hip.require_device(x, 'x')
        kind = self._kind()
        tr = None if kind is None else row_times(t, x)
        if tr is None:
            t = torch.as_tensor(t, device=x.device)
            w = torch.tanh(self.temperature * t)                                     # activations.py:149-150
            return x * (1 - w) + self.activation(x) * w
        if graph_wanted(self, x, t):
            x2, _, lead = graph_rows(x)
            return TimeMixOp.apply(x2, tr, self.temperature, kind, self._temperature_value()).reshape(*lead, x2.shape[1])
        return run_pointwise_time(x, tr, kind, self._temperature_value())[0]

    def inverse(self, y, **kwargs):
        raise NotImplementedError

    def log_diag_jacobian(self, x, y, **kwargs):
        raise NotImplementedError

    def log_det_jacobian(self, x, y, **kwargs):
        raise NotImplementedError
