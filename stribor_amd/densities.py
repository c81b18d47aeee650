"""Base densities with parameters (reference: stribor/dist/normal.py:8-37, 57-68 and stribor/dist/uniform.py:8-52 -> torch
Independent(Normal | Uniform, 1) and torch MultivariateNormal).  The package exports them from ``stribor_amd.dist`` and from the top
level, beside ``UnitNormal`` (stribor_amd/dist/normal.py), the parameter-free density of the fused kernel's epilogue.

They are nn.Modules so that ``flow.to(device)`` moves them (the reference pins them to the CPU, quirk Q6).  ``Normal``,
``MultivariateNormal`` and ``Uniform`` carry parameters: an ``nn.Parameter`` handed to the constructor is
registered as a parameter (it trains and appears in ``flow.parameters()``), anything else becomes a non-persistent buffer (the
reference's distributions contribute no ``state_dict`` keys).  ``log_prob`` is one launch of ``sx_base_logprob`` / ``sx_mvn_logprob``
(csrc/sx_base.hip) for parameters that broadcast to one vector of the row's width (an unbatched loc / matrix up to 128 columns for the
multivariate normal) on fp32 or bf16 rows; anything else -- batch-shaped parameters, the element-wise ``float`` form, wider
multivariate normals, a multivariate normal with a graph -- is ``log_prob_closed_form``: the same formulas as torch ops on the device.

Deviation: ``log_prob`` never validates the sample (the reference's default does, at one device synchronisation per call).  A sample
outside a Uniform's support gives -inf in its row -- torch's own arithmetic under ``validate_args=False`` --, a NaN gives NaN in its
row.  The PARAMETERS are validated at construction as torch does (one host synchronisation; ``validate_args=False`` skips it).
Sampling uses torch's device RNG.
"""
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _hip
from .dist.normal import UnitNormal
from .fused import ProgramCache

HALF_LOG_2PI = 0.9189385332046727          # log sqrt(2 pi)


# ---- what Normal, Uniform and MultivariateNormal share -----------------------------------------------------------------------------
def _shape(sample_shape) -> tuple:
    return (sample_shape,) if isinstance(sample_shape, int) else tuple(sample_shape)


def _work_dtype(x: torch.Tensor) -> torch.dtype:
    """fp64 rows are evaluated in fp64, everything else (fp32, bf16 storage) in fp32."""
    return torch.float64 if x.dtype == torch.float64 else torch.float32


class _ParamDist(nn.Module):
    """A density with parameters.  Subclasses: `_closed_form(x)` (torch ops, any device and dtype, differentiable), `_kernel_rows(x2,
    ldj)` ([n, D] fp32 | bf16 rows on the device + the flow's log-det [n] | None -> fp32 [n], or None outside the kernel's coverage)
    and, for calls that build a graph, `_graph_rows(x2)` (fp32 rows -> [n] with a graph, or None)."""

    def _register(self, name: str, value, like=None):
        """An nn.Parameter stays a parameter; anything else becomes a non-persistent buffer (no state_dict key)."""
        if isinstance(value, nn.Parameter):
            self.register_parameter(name, value)
            return
        if not torch.is_tensor(value):
            value = torch.tensor(float(value), dtype=torch.get_default_dtype() if like is None else like.dtype)
        elif not value.is_floating_point():
            value = value.to(torch.get_default_dtype())
        self.register_buffer(name, value.detach().clone(), persistent=False)

    def _plan_guards(self) -> list:
        return list(self.parameters(recurse=False)) + list(self.buffers(recurse=False))

    def _cached(self, key, build, tensors):
        """build() once per version of `tensors`: guarded on their (data_ptr, _version) and on the objects themselves (module.to()
        and .double() replace buffers)."""
        return self._operands.get(key, build, tensors, tuple(map(id, tensors)))

    def _wants_grad(self, x) -> bool:
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _kernel_rows(self, x2, ldj):
        return None

    def _graph_rows(self, x2):
        return None

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        """[..., D] -> [...] (element-wise for the `float` form, as the reference's reinterpreted_batch_ndims = 0).  The sample is
        not validated (module docstring)."""
        _hip.require_device(x, 'x')
        if x.dim() >= 1 and x.numel() > 0 and x.dtype in (torch.float32, torch.bfloat16):
            if self._wants_grad(x):
                out = self._graph_rows(x.reshape(-1, x.shape[-1]).to(torch.float32))
            else:
                out = self._kernel_rows(x.reshape(-1, x.shape[-1]).contiguous(), None)
            if out is not None:
                return out.reshape(x.shape[:-1])
        return self._closed_form(x)

    def forward(self, x):
        return self.log_prob(x)

    def sample(self, sample_shape=()) -> torch.Tensor:
        with torch.no_grad():
            return self.rsample(sample_shape)


def log_prob_closed_form(dist, x: torch.Tensor) -> torch.Tensor:
    """log_prob of a Normal / Uniform / MultivariateNormal / UnitNormal as torch ops on x's device, in fp64 for fp64 rows and in fp32
    otherwise: the formulas of torch.distributions in their order (dist/normal.py:37, dist/uniform.py:36), differentiable, no sample
    validation.  What `log_prob` evaluates outside the kernels' coverage, and what the host tests hold to the reference's values."""
    if isinstance(dist, UnitNormal):
        xf = x.to(_work_dtype(x))
        return (-(xf ** 2) / 2 - HALF_LOG_2PI).sum(-1)
    return dist._closed_form(x)


def _vector(t: torch.Tensor, d: int):
    """t broadcast to one vector [d] (a view with t's graph), or None when t has a batch shape."""
    if t.numel() == 1:
        return t.reshape(1).expand(d)
    if t.numel() == d and t.shape[-1] == d:
        return t.reshape(d)
    return None


def _f32c(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


# ---- Normal ------------------------------------------------------------------------------------------------------------------------
class _NormalLogProb(torch.autograd.Function):
    """log_prob of fp32 rows under Normal(loc [D], scale [D]) as a once-differentiable op: forward sx_base_logprob, backward
    sx_normal_logprob_bwd (dx and the two column sums in one pass, per-block partials in slot order: the same bits every call)."""

    @staticmethod
    def forward(ctx, x2, loc, scale):
        x2 = x2.contiguous()
        s64 = scale.detach().to(x2.device, torch.float64)
        loc, inv = _f32c(loc, x2.device), (1.0 / s64).to(torch.float32).contiguous()
        out = torch.empty(x2.shape[0], dtype=torch.float32, device=x2.device)
        _hip.call('sx_base_logprob', x2, x2.data_ptr(), loc.data_ptr(), inv.data_ptr(), 0.0, None, out.data_ptr(),
                  x2.shape[0], x2.shape[1], _hip.SX_F32, _hip.BASE_NORMAL)
        # the constant -sum log scale - D log sqrt(2 pi) stays on the device here (fp64, rounded once, added as the kernel would add
        # it): the parameters change every training step, and a host constant would cost a synchronisation per step
        out += (-s64.log().sum() - x2.shape[1] * HALF_LOG_2PI).to(torch.float32)
        ctx.save_for_backward(x2, loc, inv)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x2, loc, inv = ctx.saved_tensors
        n, d = x2.shape
        want_x, want_loc, want_scale = ctx.needs_input_grad[:3]
        g = g.to(torch.float32).contiguous()
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x2.device)
        gx = new(n, d) if want_x else None
        g_loc = new(d) if want_loc else None
        g_scale = new(d) if want_scale else None
        partial = new(max(int(_hip.lib().sx_normal_bwd_partial_floats(n, d)), 1)) if (want_loc or want_scale) else None
        _hip.call('sx_normal_logprob_bwd', x2, x2.data_ptr(), g.data_ptr(), loc.data_ptr(), inv.data_ptr(), _hip.ptr(gx), _hip.ptr(g_loc),
                  _hip.ptr(g_scale), _hip.ptr(partial), n, d)
        # (the constant's share of d scale, -g / scale, is in the kernel)
        return gx, g_loc, g_scale


class Normal(_ParamDist):
    """st.Normal(loc, scale) (dist/normal.py:8-37): tensors -> log_prob sums over the last axis; a Python `float` loc -> element-wise
    (the reference's `isinstance(self.loc, float)`; an `int` is not a float there, and a scalar density then has no axis to sum over:
    ValueError)."""

    def __init__(self, loc, scale, validate_args=None, **kwargs):
        super().__init__()
        self.elementwise = isinstance(loc, float)
        like = next((t for t in (loc, scale) if torch.is_tensor(t) and t.is_floating_point()), None)
        self._register('loc', loc, like)
        self._register('scale', scale, like)
        shape = torch.broadcast_shapes(self.loc.shape, self.scale.shape)
        if not self.elementwise and len(shape) == 0:
            raise ValueError('Normal: scalar parameters that are not a Python float have no event axis to sum over '
                             '(pass loc as a float for the element-wise form, or tensors of shape [..., D])')
        self.dim = None if self.elementwise or len(shape) == 0 else int(shape[-1])
        if validate_args is not False and not bool((self.scale.detach() > 0).all()):
            raise ValueError('Normal: `scale` must be positive')
        self._operands = ProgramCache()

    def _params(self, dtype=None):
        loc, scale = torch.broadcast_tensors(self.loc, self.scale)
        return (loc, scale) if dtype is None else (loc.to(dtype), scale.to(dtype))

    def _closed_form(self, x):
        dt = _work_dtype(x)
        loc, scale = self._params(dt)
        lp = -((x.to(dt) - loc) ** 2) / (2 * scale ** 2) - scale.log() - math.log(math.sqrt(2 * math.pi))    # torch Normal.log_prob
        return lp if self.elementwise else lp.sum(-1)

    def _vectors(self, d: int):
        if self.elementwise:
            return None
        loc, scale = _vector(self.loc, d), _vector(self.scale, d)
        return None if loc is None or scale is None else (loc, scale)

    def _log_norm(self, d: int, device) -> float:
        """-sum log scale - D log sqrt(2 pi) in fp64 on the host: one read-back per parameter version."""
        def build():
            s = _vector(self.scale, d).detach().double().cpu()
            return float(-s.log().sum().item() - d * HALF_LOG_2PI)
        return self._cached(('log-norm', d), build, [self.scale])

    def _kernel_operands(self, d: int, device):
        def build():
            loc, scale = self._vectors(d)
            return _f32c(loc, device), (1.0 / scale.detach().to(device, torch.float64)).to(torch.float32).contiguous()
        return self._cached(('operands', d, str(device)), build, [self.loc, self.scale])

    def _kernel_rows(self, x2, ldj):
        d = x2.shape[1]
        if self._vectors(d) is None:
            return None
        loc, inv = self._kernel_operands(d, x2.device)
        out = torch.empty(x2.shape[0], dtype=torch.float32, device=x2.device)
        _hip.call('sx_base_logprob', x2, x2.data_ptr(), loc.data_ptr(), inv.data_ptr(), self._log_norm(d, x2.device), _hip.ptr(ldj),
                  out.data_ptr(), x2.shape[0], d, _hip.dtype_code(x2), _hip.BASE_NORMAL)
        return out

    def _graph_rows(self, x2):
        v = self._vectors(x2.shape[1])
        if v is None:
            return None
        return _NormalLogProb.apply(x2, v[0].to(x2.device, torch.float32), v[1].to(x2.device, torch.float32))

    def _plan(self, builder) -> bool:
        """The density as the last step of a log_prob program: what Affine(dim, scale=scale, shift=loc) plans in that direction
        (z = (x - loc) / scale, log-det -sum log scale) in front of the kernel's unit-normal epilogue."""
        v = self._vectors(builder.dim)
        if v is None:
            return False
        d = builder.dim

        def derive(dev):
            loc, scale = self._vectors(d)
            return scale.detach().to(dev, torch.float64).log().to(torch.float32), _f32c(loc, dev)
        builder.add_affine_const(self.scale, self.loc, reverse=True, ldj_scale=-1.0, derive=derive)
        return True

    # ---- torch.distributions surface ----
    @property
    def mean(self):
        return self._params()[0]

    @property
    def stddev(self):
        return self._params()[1]

    @property
    def variance(self):
        return self._params()[1] ** 2

    def entropy(self):
        h = 0.5 + 0.5 * math.log(2 * math.pi) + self._params()[1].log()
        return h if self.elementwise else h.sum(-1)

    def rsample(self, sample_shape=()) -> torch.Tensor:
        loc, scale = self._params()
        return loc + scale * torch.randn(_shape(sample_shape) + tuple(loc.shape), dtype=loc.dtype, device=loc.device)


# ---- MultivariateNormal ------------------------------------------------------------------------------------------------------------
class MultivariateNormal(_ParamDist):
    """st.MultivariateNormal(loc, covariance_matrix | precision_matrix | scale_tril) (dist/normal.py:57-68).  The lower-triangular
    factor L is derived in fp64; the kernel takes L^-1 rounded once to fp32."""

    def __init__(self, loc, covariance_matrix=None, precision_matrix=None, scale_tril=None, validate_args=None, **kwargs):
        super().__init__()
        given = [(n, m) for n, m in (('covariance_matrix', covariance_matrix), ('precision_matrix', precision_matrix),
                                     ('scale_tril', scale_tril)) if m is not None]
        if len(given) != 1:
            raise ValueError('Exactly one of covariance_matrix or precision_matrix or scale_tril may be specified.')
        self._matrix_name, matrix = given[0]
        if not torch.is_tensor(loc) or loc.dim() < 1:
            raise ValueError('loc must be at least one-dimensional.')
        if not torch.is_tensor(matrix) or matrix.dim() < 2 or matrix.shape[-1] != matrix.shape[-2] or matrix.shape[-1] != loc.shape[-1]:
            raise ValueError(f'{self._matrix_name} must be at least two-dimensional, [..., D, D] with D = loc.shape[-1]')
        self._register('loc', loc)
        self._register(self._matrix_name, matrix)
        self.dim = int(loc.shape[-1])
        if validate_args is not False:
            m = matrix.detach().double()
            if self._matrix_name == 'scale_tril':
                ok = bool((m.tril() == m).all()) and bool((m.diagonal(dim1=-2, dim2=-1) > 0).all())
            else:
                ok = bool(torch.isclose(m, m.mT, atol=1e-6).all()) and bool((torch.linalg.cholesky_ex(m).info == 0).all())
            if not ok:
                raise ValueError(f'MultivariateNormal: `{self._matrix_name}` must be '
                                 + ('lower-triangular with a positive diagonal' if self._matrix_name == 'scale_tril' else 'positive-definite'))
        self._operands = ProgramCache()

    @property
    def _matrix(self):
        return getattr(self, self._matrix_name)

    def _tril64(self) -> torch.Tensor:
        """L in fp64 from the module's matrix, with its graph (torch MultivariateNormal.__init__ / _precision_to_scale_tril)."""
        m = self._matrix.double()
        if self._matrix_name == 'scale_tril':
            return m
        if self._matrix_name == 'covariance_matrix':
            return torch.linalg.cholesky(m)
        lf = torch.linalg.cholesky(torch.flip(m, (-2, -1)))
        l_inv = torch.transpose(torch.flip(lf, (-2, -1)), -2, -1)
        eye = torch.eye(m.shape[-1], dtype=m.dtype, device=m.device)
        return torch.linalg.solve_triangular(l_inv, eye, upper=False)

    def _closed_form(self, x):
        dt = _work_dtype(x)
        L = self._tril64().to(dt)
        diff = x.to(dt) - self.loc.to(dt)
        z = torch.linalg.solve_triangular(L, diff.unsqueeze(-1), upper=False).squeeze(-1)
        half_log_det = L.diagonal(dim1=-2, dim2=-1).log().sum(-1)
        return -0.5 * (self.dim * math.log(2 * math.pi) + (z ** 2).sum(-1)) - half_log_det       # torch MultivariateNormal.log_prob

    def _unbatched(self) -> bool:
        return self.loc.dim() == 1 and self._matrix.dim() == 2

    def _derived(self, device):
        """-> (Linv fp64 [D, D], loc fp64 [D], sum log L_ii fp64 0-dim) on the device, once per parameter version."""
        def build():
            with torch.no_grad():
                L = self._tril64().to(device).contiguous()
                d = self.dim
                if d <= 128 and L.is_cuda:
                    linv = torch.zeros_like(L)
                    _hip.call('sx_tri_inverse_f64', L, L.data_ptr(), linv.data_ptr(), 1, d, 1, 0)
                else:
                    linv = torch.linalg.solve_triangular(L, torch.eye(d, dtype=L.dtype, device=L.device), upper=False)
                return linv, self.loc.detach().to(device, torch.float64), L.diagonal().log().sum()
        return self._cached(('derived', str(device)), build, [self.loc, self._matrix])

    def _kernel_operands(self, device):
        def build():
            linv, loc, log_det = self._derived(device)
            # (log_norm travels as a host constant: one read-back per parameter version)
            return linv.to(torch.float32).contiguous(), loc.to(torch.float32).contiguous(), float(-log_det.item() - self.dim * HALF_LOG_2PI)
        return self._cached(('operands', str(device)), build, [self.loc, self._matrix])

    def _kernel_rows(self, x2, ldj):
        if not self._unbatched() or self.dim > _hip.MVN_MAX_DIM or x2.shape[1] != self.dim:
            return None
        linv, loc, log_norm = self._kernel_operands(x2.device)
        out = torch.empty(x2.shape[0], dtype=torch.float32, device=x2.device)
        _hip.call('sx_mvn_logprob', x2, x2.data_ptr(), loc.data_ptr(), linv.data_ptr(), log_norm, _hip.ptr(ldj), out.data_ptr(),
                  x2.shape[0], self.dim, _hip.dtype_code(x2))
        return out

    def _plan(self, builder) -> bool:
        """The density as the last step of a log_prob program: the dense layer z = Linv x - Linv loc with log-det -sum log L_ii in
        front of the kernel's unit-normal epilogue."""
        if not self._unbatched() or builder.dim != self.dim:
            return False

        def fn(dev):
            linv, loc, _ = self._derived(dev)
            return linv, -(linv @ loc)
        builder.add_linear([self.loc, self._matrix], fn, lambda dev: -self._derived(dev)[2])
        return True

    # ---- torch.distributions surface ----
    @property
    def mean(self):
        return self.loc

    @property
    def variance(self):
        return (self._tril64() ** 2).sum(-1).to(self.loc.dtype).expand(torch.broadcast_shapes(self.loc.shape, self._matrix.shape[:-1]))

    def entropy(self):
        half_log_det = self._tril64().diagonal(dim1=-2, dim2=-1).log().sum(-1)
        return (0.5 * self.dim * (1.0 + math.log(2 * math.pi)) + half_log_det).to(self.loc.dtype)

    def rsample(self, sample_shape=()) -> torch.Tensor:
        L = self._tril64().to(self.loc.dtype)
        batch = torch.broadcast_shapes(self.loc.shape[:-1], L.shape[:-2])
        eps = torch.randn(_shape(sample_shape) + tuple(batch) + (self.dim,), dtype=self.loc.dtype, device=self.loc.device)
        return self.loc + (L @ eps.unsqueeze(-1)).squeeze(-1)


# ---- Uniform (the support is low <= x < high) ------------------------------------------------------------------------------------
class _UniformLogProb(torch.autograd.Function):
    """log_prob of fp32 rows under Uniform(low [D], high [D]) as a once-differentiable op.  The backward needs no kernel: dx = 0,
    d low = sum_n g_n / (high - low), d high = -d low (the support's indicator has no gradient, as in torch)."""

    @staticmethod
    def forward(ctx, x2, low, high):
        x2 = x2.contiguous()
        lo, hi = _f32c(low, x2.device), _f32c(high, x2.device)
        out = torch.empty(x2.shape[0], dtype=torch.float32, device=x2.device)
        _hip.call('sx_base_logprob', x2, x2.data_ptr(), lo.data_ptr(), hi.data_ptr(), 0.0, None, out.data_ptr(),
                  x2.shape[0], x2.shape[1], _hip.SX_F32, _hip.BASE_UNIFORM)
        # (the constant -sum log(high - low) on the device, as in _NormalLogProb: no synchronisation per training step)
        out += (-(high.detach().to(x2.device, torch.float64) - low.detach().to(x2.device, torch.float64)).log().sum()).to(torch.float32)
        ctx.save_for_backward(lo, hi)
        ctx.x_shape = x2.shape
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lo, hi = ctx.saved_tensors
        want_x, want_low, want_high = ctx.needs_input_grad[:3]
        g_low = g.to(torch.float32).sum() / (hi - lo) if (want_low or want_high) else None
        return (torch.zeros(ctx.x_shape, dtype=torch.float32, device=lo.device) if want_x else None,
                g_low if want_low else None, -g_low if want_high else None)


class Uniform(_ParamDist):
    """st.Uniform(low, high) (dist/uniform.py:8-36): tensors -> log_prob sums over the last axis; a Python `float` low ->
    element-wise (the reference's `isinstance(self.low, float)`; an `int` is not a float there, and a scalar density then has no
    axis to sum over: ValueError)."""

    def __init__(self, low, high, validate_args=None, **kwargs):
        super().__init__()
        self.elementwise = isinstance(low, float)
        like = next((t for t in (low, high) if torch.is_tensor(t) and t.is_floating_point()), None)
        self._register('low', low, like)
        self._register('high', high, like)
        shape = torch.broadcast_shapes(self.low.shape, self.high.shape)
        if not self.elementwise and len(shape) == 0:
            raise ValueError('Uniform: scalar bounds that are not a Python float have no event axis to sum over '
                             '(pass low as a float for the element-wise form, or tensors of shape [..., D])')
        self.dim = None if self.elementwise or len(shape) == 0 else int(shape[-1])
        if validate_args is not False and not bool((self.low.detach() < self.high.detach()).all()):
            raise ValueError('Uniform: `low` must be smaller than `high`')
        self._operands = ProgramCache()

    def _params(self, dtype=None):
        low, high = torch.broadcast_tensors(self.low, self.high)
        return (low, high) if dtype is None else (low.to(dtype), high.to(dtype))

    def _closed_form(self, x):
        dt = _work_dtype(x)
        low, high = self._params(dt)
        x = x.to(dt)
        lb = low.le(x).type_as(low)
        ub = high.gt(x).type_as(low)
        lp = torch.log(lb.mul(ub)) - torch.log(high - low)                       # torch Uniform.log_prob
        lp = torch.where(torch.isnan(x), x, lp)                                  # (a NaN stays a NaN: module docstring, deviation)
        return lp if self.elementwise else lp.sum(-1)

    def _vectors(self, d: int):
        if self.elementwise:
            return None
        low, high = _vector(self.low, d), _vector(self.high, d)
        return None if low is None or high is None else (low, high)

    def _log_norm(self, d: int) -> float:
        """-sum log(high - low) in fp64 on the host: one read-back per parameter version."""
        def build():
            low, high = self._vectors(d)
            return float(-(high.detach().double() - low.detach().double()).log().sum().item())
        return self._cached(('log-norm', d), build, [self.low, self.high])

    def _kernel_rows(self, x2, ldj):
        d = x2.shape[1]
        if self._vectors(d) is None:
            return None

        def build():
            low, high = self._vectors(d)
            return _f32c(low, x2.device), _f32c(high, x2.device)
        lo, hi = self._cached(('operands', d, str(x2.device)), build, [self.low, self.high])
        out = torch.empty(x2.shape[0], dtype=torch.float32, device=x2.device)
        _hip.call('sx_base_logprob', x2, x2.data_ptr(), lo.data_ptr(), hi.data_ptr(), self._log_norm(d), _hip.ptr(ldj), out.data_ptr(),
                  x2.shape[0], d, _hip.dtype_code(x2), _hip.BASE_UNIFORM)
        return out

    def _graph_rows(self, x2):
        v = self._vectors(x2.shape[1])
        if v is None:
            return None
        return _UniformLogProb.apply(x2, v[0].to(x2.device, torch.float32), v[1].to(x2.device, torch.float32))

    # ---- torch.distributions surface ----
    @property
    def mean(self):
        low, high = self._params()
        return (high + low) / 2

    @property
    def stddev(self):
        low, high = self._params()
        return (high - low) / 12 ** 0.5

    @property
    def variance(self):
        low, high = self._params()
        return (high - low) ** 2 / 12

    def entropy(self):
        low, high = self._params()
        h = torch.log(high - low)
        return h if self.elementwise else h.sum(-1)

    def rsample(self, sample_shape=()) -> torch.Tensor:
        low, high = self._params()
        return low + torch.rand(_shape(sample_shape) + tuple(low.shape), dtype=low.dtype, device=low.device) * (high - low)


class UnitUniform(Uniform):
    """st.UnitUniform(dim) (dist/uniform.py:38-52): Uniform on [0, 1)^dim."""

    def __init__(self, dim: int):
        super().__init__(torch.zeros(dim), torch.ones(dim))
        self.dim = dim
