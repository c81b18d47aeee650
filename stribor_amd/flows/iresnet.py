"""Invertible ResNet flows (reference: stribor/flows/iresnet.py:9-99): ``IResNet`` and ``ContinuousIResNet``.

Same constructors, same ``state_dict`` keys (``net.net.0.weight``, ``net.net.2.weight_orig / weight_u / weight_v``, ...,
``time_net.*``), same construction order and RNG draws: the residual network is the product ``net.MLP`` with every Linear
after the first wrapped in ``torch.nn.utils.spectral_norm`` (mlp.py:46-50).

Without an autograd graph, ``forward`` and the fixed-point ``inverse`` are ONE launch of ``sx_resnet_flow`` (the row state and
the hidden activations stay in registers for all iterations, the weights sit in LDS), preceded by one launch of
``sx_spectral_sigma``, which advances the spectral-norm vectors exactly as the reference's hooks would (one hook call per
evaluation of the network: ``iterations`` calls for an inverse in training mode, each with its own sigma) and writes the table
of sigmas the flow kernel scales by.  Networks outside the kernel's coverage (a custom activation, layers wider than 128, more
than three hidden layers, weights over the LDS budget) run the same schedule as a composition of the product MLP and torch
element-wise ops.

With an autograd graph (training), networks inside ``sx_resnet_flow_bwd``'s coverage (``_train_plan``: dim and widths <= 64, the
images within the LDS budget) keep both directions on the kernels: ``_ForwardFn`` / ``_InverseFn`` run the same forward launches
and ONE ``sx_resnet_flow_bwd`` call in backward -- the vector-Jacobian product, or the whole implicit-function iteration of the
inverse, with the weight gradients contracted in-kernel.  s = time_net(t) is evaluated by torch outside the Function and enters
it as a tensor, so t and any time net's parameters get their gradients from autograd.  Everything else composes torch ops as
before; ``_last_grad_path`` says which of the two a graph-building call took.
"""
import ctypes
from typing import List, Optional

import torch
import torch.nn as nn
from torch.nn.utils.spectral_norm import SpectralNorm

from .. import _hip
from ..flow import Transform, flatten_rows, graph_wanted
from ..net.cover import linear_stack
from ..net.mlp import MLP
from ..net.time_net import TimeFourier, TimeIdentity, TimeLinear, TimeLog, TimeTanh

__all__ = ['IResNet', 'ContinuousIResNet']


def _sn_hook(layer: nn.Module):
    for h in layer._forward_pre_hooks.values():
        if isinstance(h, SpectralNorm):
            return h
    return None


def _time_kind(tn) -> Optional[int]:
    """The in-kernel time-embedding kind of `tn` (SX_RESNET_TIME_*), or None (then s = time_net(t) is passed as rows)."""
    if type(tn) in (TimeIdentity,):
        return 0
    if type(tn) in (TimeLinear, TimeTanh, TimeLog):
        return tn.kind
    if isinstance(tn, TimeFourier) and type(tn).forward is TimeFourier.forward:
        return 4
    return None


def spectral_weight_grad(G, W_orig, u, v, sigma):
    """dL/dW_orig of the spectrally normalised weight W_orig / sigma, sigma = u . (W_orig v) with u and v held constant (what
    torch.nn.utils.spectral_norm differentiates), from G = dL/d(W_orig / sigma): G / sigma - (<G, W_orig> / sigma^2) u v^T."""
    return G / sigma - (torch.sum(G * W_orig) / (sigma * sigma)) * torch.outer(u, v)


def _param_grads(module, wrapped_uv, sigma, G, db, spec):
    """The kernel's G_l / db_l carried to the module's parameters, in the order of `spec` [(layer, 'W' | 'b')]."""
    out = []
    for i, kind in spec:
        if kind == 'b':
            out.append(db[i])
        elif G[i] is None:
            out.append(None)
        elif i in wrapped_uv:
            col, W_orig, u, v = wrapped_uv[i]
            out.append(spectral_weight_grad(G[i], W_orig, u, v, sigma[0, col]))
        else:
            out.append(G[i])
    return out


class _ForwardFn(torch.autograd.Function):
    """y = x + s * g(x) on the kernels: the no-graph forward (``sx_spectral_sigma`` -- in training mode u / v advance once, as the
    hook would -- and ``sx_resnet_flow``), and in backward one ``sx_resnet_flow_bwd`` call at the sigma, u and v of THIS call.
    Entered with grad mode on (create_graph), backward recomputes through torch ops and returns a differentiable result."""

    @staticmethod
    def forward(ctx, module, x2, s, *params):
        plan = module._train_plan()
        d, keep, wrapped = plan
        with torch.no_grad():
            sigma, rows = module._sigma_table(wrapped, 1, x2)
            y = module._run_rows(x2, None, 1, False, s=s, plan=plan, sigma=(sigma, rows))
        ctx.module, ctx.sigma, ctx.has_s = module, sigma, s is not None
        ctx.uv = [(lin.weight_u.detach().clone(), lin.weight_v.detach().clone()) for lin, _ in wrapped]
        ctx.save_for_backward(x2, *(() if s is None else (s,)), *params)
        return y

    @staticmethod
    def backward(ctx, gy):
        saved = ctx.saved_tensors
        x2 = saved[0]
        s = saved[1] if ctx.has_s else None
        m = ctx.module
        needs = ctx.needs_input_grad
        n_params = len(saved) - 1 - int(ctx.has_s)
        if torch.is_grad_enabled():
            params = list(saved[1 + int(ctx.has_s):])
            y = x2 + m._residual_at(x2, s, ctx.uv)
            wanted = [(1, x2)] * bool(needs[1]) + [(2, s)] * bool(needs[2] and s is not None)
            wanted += [(3 + i, p) for i, p in enumerate(params) if needs[3 + i]]
            got = torch.autograd.grad(y, [w for _, w in wanted], gy, create_graph=True, allow_unused=True) if wanted else ()
            out = [None] * (3 + n_params)
            for (k, _), g in zip(wanted, got):
                out[k] = g
            return tuple(out)
        plan = m._train_plan()
        spec = m._param_spec()
        gx, gs, grads = m._kernel_backward(plan, x2, s, ctx.sigma, ctx.uv, gy, 0, False, bool(needs[2]) and s is not None,
                                           [needs[3 + i] for i in range(n_params)], spec)
        return (None, gx if needs[1] else None, gs, *grads)


class _InverseFn(torch.autograd.Function):
    """The fixed-point inverse on the kernels, with the implicit-function backward of ``_InverseComposedFn`` as ONE
    ``sx_resnet_flow_bwd`` call: w <- gx - J_r(x*)^T w for `iterations` steps, dL/dy = w, the cotangents of s and of the network's
    parameters at -w.  sigma, u and v are frozen at their values when backward runs (a sigma row from ``sx_spectral_sigma`` with no
    power iteration), as ``_frozen_weight`` does."""

    @staticmethod
    def forward(ctx, module, y2, s, iterations, *params):
        with torch.no_grad():
            x = module._run_rows(y2, None, iterations, True, s=s, plan=module._train_plan())
        ctx.module, ctx.iterations, ctx.has_s = module, iterations, s is not None
        ctx.save_for_backward(x, *(() if s is None else (s,)), *params)
        return x

    @staticmethod
    def backward(ctx, gx):
        saved = ctx.saved_tensors
        x = saved[0]
        s = saved[1] if ctx.has_s else None
        m = ctx.module
        needs = ctx.needs_input_grad
        n_params = len(saved) - 1 - int(ctx.has_s)
        p_needs = [needs[4 + i] for i in range(n_params)]
        want_s = bool(needs[2]) and s is not None
        if torch.is_grad_enabled():                       # higher-order use: the torch restatement of the same iteration
            params = list(saved[1 + int(ctx.has_s):])
            with torch.enable_grad():
                xr = x.detach().requires_grad_(True)
                sr = None if s is None else s.detach().requires_grad_(want_s)
                r = m._residual_at(xr, sr, None)
                w = gx
                for _ in range(ctx.iterations):
                    (jtw,) = torch.autograd.grad(r, xr, w, retain_graph=True)
                    w = gx - jtw
                wanted = [sr] * want_s + [p for p, k in zip(params, p_needs) if k]
                got = list(torch.autograd.grad(r, wanted, w, allow_unused=True)) if wanted else []
            got = [None if g is None else -g for g in got]
            gs = got.pop(0) if want_s else None
            return (None, w, gs, None, *[got.pop(0) if k else None for k in p_needs])
        plan = m._train_plan()
        d, keep, wrapped = plan
        with torch.no_grad():
            sigma, _ = m._sigma_table(wrapped, 1, x, frozen=True)
        uv = [(lin.weight_u.detach(), lin.weight_v.detach()) for lin, _ in wrapped]
        gy, gs, grads = m._kernel_backward(plan, x, s, sigma, uv, gx, ctx.iterations, True, want_s, p_needs, m._param_spec())
        return (None, gy, gs, None, *grads)


class _InverseComposedFn(torch.autograd.Function):
    """The fixed-point inverse with an implicit-function backward, for networks outside ``_train_plan``.

    Forward: the no-graph inverse (one ``sx_resnet_flow`` launch).  Backward, at the fixed point x* = y - r(x*), r = s * g:
    w <- gx - J_r(x*)^T w for `iterations` steps from w = gx, then dL/dy = w, dL/dtheta = -(dr/dtheta)^T w (theta: t, the
    network's weight_orig / biases -- sigma = u . (W_orig v) included -- and the time net's parameters).  This equals the
    reference's gradient through its unrolled loop up to the loop's convergence error; where sigma moves between iterations
    (training mode) r is taken with the LAST iteration's sigma."""

    @staticmethod
    def forward(ctx, module, y2, t2, iterations, *params):
        with torch.no_grad():
            x = module._inverse_rows(y2, t2, iterations)
        ctx.module, ctx.iterations, ctx.n_params = module, iterations, len(params)
        ctx.has_t = t2 is not None
        ctx.save_for_backward(x, *(() if t2 is None else (t2,)), *params)
        return x

    @staticmethod
    def backward(ctx, gx):
        saved = ctx.saved_tensors
        x = saved[0]
        t2 = saved[1] if ctx.has_t else None
        params = list(saved[1 + int(ctx.has_t):])
        m = ctx.module
        with torch.enable_grad():
            xr = x.detach().requires_grad_(True)
            tr = None
            want = []
            if t2 is not None:
                tr = t2.detach().requires_grad_(ctx.needs_input_grad[2])
                if ctx.needs_input_grad[2]:
                    want.append(tr)
            r = m._residual(xr, tr, frozen=True)
            w = gx
            for _ in range(ctx.iterations):
                (jtw,) = torch.autograd.grad(r, xr, w, retain_graph=True)
                w = gx - jtw
            p_want = [p for i, p in enumerate(params) if ctx.needs_input_grad[4 + i]]
            grads = torch.autograd.grad(r, want + p_want, w, allow_unused=True) if (want or p_want) else ()
        grads = [None if g is None else -g for g in grads]
        gt = grads.pop(0) if want else None
        out_p = []
        for i, p in enumerate(params):
            out_p.append(grads.pop(0) if ctx.needs_input_grad[4 + i] else None)
        if gt is None and tr is not None and ctx.needs_input_grad[2]:
            gt = torch.zeros_like(t2)
        return (None, w, gt, None, *out_p)


class _IResNetBase(Transform):
    def _make_net(self, dim, hidden_dims, activation, final_activation, n_power_iterations):
        wrapper = lambda layer: nn.utils.spectral_norm(layer, n_power_iterations=n_power_iterations)    # iresnet.py:31, 76
        self.dim = dim
        self.net = MLP(dim, hidden_dims, dim, activation, final_activation, nn_linear_wrapper_func=wrapper)

    # ---- the pieces -----------------------------------------------------------------------------------------------------
    def _time(self):
        return getattr(self, 'time_net', None)

    def _s(self, t2, n, dtype_device_like):
        """s = time_net(t) as [n, dim] (torch ops; differentiable), or None for IResNet."""
        tn = self._time()
        if tn is None:
            return None
        s = tn(t2)
        return s.expand(n, self.dim) if s.shape != (n, self.dim) else s

    def _g_torch(self, x2):
        """g(x) through the product MLP's torch layers: every wrapped Linear runs its spectral-norm hook (a power iteration in
        training mode, as in the reference)."""
        return self.net.net(x2)

    def _frozen_weight(self, lin):
        """weight_orig / sigma with sigma = u . (W_orig v) at the CURRENT u, v (no power iteration; differentiable in W_orig)."""
        hook = _sn_hook(lin)
        if hook is None:
            return lin.weight
        W = getattr(lin, hook.name + '_orig')
        u = getattr(lin, hook.name + '_u').detach().clone()
        v = getattr(lin, hook.name + '_v').detach().clone()
        Wm = hook.reshape_weight_to_matrix(W)
        return W / torch.dot(u, torch.mv(Wm, v))

    def _residual(self, x2, t2, frozen: bool):
        """r = s * g(x) with a graph.  frozen: the spectral-norm weights at the current u, v (the backward of the inverse);
        otherwise the hooks run (forward with a graph)."""
        if frozen:
            h = x2
            for layer in self.net.net:
                h = nn.functional.linear(h, self._frozen_weight(layer), layer.bias) if isinstance(layer, nn.Linear) else layer(h)
            g = h
        else:
            g = self._g_torch(x2)
        s = self._s(t2, x2.shape[0], x2) if t2 is not None else None
        return g if s is None else s * g

    def _residual_at(self, x2, s, uv):
        """r = s * g(x) in torch ops with s given and the spectral-norm weights at `uv` [(u, v) per wrapped layer] (None: the
        current ones); differentiable in x, s and the parameters."""
        h, j = x2, 0
        for layer in self.net.net:
            if not isinstance(layer, nn.Linear):
                h = layer(h)
                continue
            hook = _sn_hook(layer)
            if hook is None or uv is None:
                W = self._frozen_weight(layer)
            else:
                W = layer.weight_orig / torch.dot(uv[j][0], torch.mv(layer.weight_orig, uv[j][1]))
            j += hook is not None
            h = nn.functional.linear(h, W, layer.bias)
        return h if s is None else s * h

    # ---- the kernel plan ---------------------------------------------------------------------------------------------------
    def _param_list(self):
        """[(parameter, (layer, 'W' | 'b'))] of the residual network, in layer order (weight_orig of a wrapped layer)."""
        out = []
        for i, lin in enumerate(m for m in self.net.net if isinstance(m, nn.Linear)):
            out.append((lin.weight_orig if _sn_hook(lin) is not None else lin.weight, (i, 'W')))
            if lin.bias is not None:
                out.append((lin.bias, (i, 'b')))
        return out

    def _param_spec(self):
        return [k for _, k in self._param_list()]

    def _train_plan(self):
        """The kernel plan of a graph-building call -- ``_kernel_net()`` for a network ``sx_resnet_flow_bwd`` covers, every tensor
        contiguous float32 -- or None (the call then composes torch ops).  Host only: works on CPU modules."""
        plan = self._kernel_net()
        if plan is None:
            return None
        d, keep, wrapped = plan
        if _hip.lib().sx_resnet_bwd_lds_bytes(d) == 0:
            return None
        for lin, _ in wrapped:
            for tsr in (lin.weight_u, lin.weight_v):
                if tsr.dtype != torch.float32 or not tsr.is_contiguous():
                    return None
        return plan

    def _kernel_backward(self, plan, x, s, sigma, uv, gin, iterations, inverse, want_s, p_needs, spec):
        """One ``sx_resnet_flow_bwd`` call -> (gout, gs | None, [parameter gradient | None] in `spec` order)."""
        d, keep, wrapped = plan
        n = x.shape[0]
        gin = gin.to(torch.float32).contiguous()
        L = d.n_layers
        want = {k: bool(w) for k, w in zip(spec, p_needs)}
        shapes = [(d.layer[i].out_dim, d.layer[i].in_dim) for i in range(L)]
        G = [torch.zeros(sh, dtype=torch.float32, device=x.device) if want.get((i, 'W')) else None for i, sh in enumerate(shapes)]
        db = [torch.zeros(sh[0], dtype=torch.float32, device=x.device) if want.get((i, 'b')) else None for i, sh in enumerate(shapes)]
        gout = torch.empty_like(x)
        gs = torch.empty_like(x) if want_s else None
        if n:
            rec = _hip.sx_resnet_grads()
            for i in range(L):
                rec.dW[i], rec.db[i] = _hip.ptr(G[i]), _hip.ptr(db[i])
            partial = None
            if any(want.values()):
                partial = torch.empty(_hip.lib().sx_resnet_bwd_partial_floats(d, n), dtype=torch.float32, device=x.device)
            _hip.call('sx_resnet_flow_bwd', x, ctypes.byref(d), x.data_ptr(), _hip.ptr(s), _hip.ptr(sigma), gin.data_ptr(), gout.data_ptr(),
                      _hip.ptr(gs), _hip.ptr(partial), ctypes.byref(rec), n, int(iterations), int(inverse))
        del keep
        wrapped_uv = {}
        lins = [m for m in self.net.net if isinstance(m, nn.Linear)]
        for col, ((lin, _), (u, v)) in enumerate(zip(wrapped, uv)):
            wrapped_uv[lins.index(lin)] = (col, lin.weight_orig.detach(), u, v)
        grads = _param_grads(self, wrapped_uv, sigma, G, db, spec)
        return gout, gs, [g if k else None for g, k in zip(grads, p_needs)]

    def _kernel_net(self):
        """(sx_resnet_net, keep-alive list, wrapped [(layer, hook)]) for the kernel, or None when the network is outside its
        coverage."""
        net = self.net
        if net.activation_name not in _hip.ACT_CODES:
            return None
        fa = net.final_activation_name
        if fa is not None and fa not in _hip.ACT_CODES:
            return None
        lins = linear_stack(net.net, final_activation=fa is not None)
        if lins is None or len(lins) > _hip.RESNET_MAX_LAYERS:
            return None
        d = _hip.sx_resnet_net()
        keep, wrapped = [], []
        for i, lin in enumerate(lins):
            hook = _sn_hook(lin)
            if hook is not None:
                if hook.name != 'weight' or hook.dim != 0:
                    return None
                W = getattr(lin, 'weight_orig')
                col = len(wrapped)
                wrapped.append((lin, hook))
            else:
                W, col = lin.weight, -1
            W = W.detach()
            b = None if lin.bias is None else lin.bias.detach()
            if W.dtype != torch.float32 or not W.is_contiguous() or W.shape[0] > 128 or W.shape[1] > 128:
                return None
            if b is not None and (b.dtype != torch.float32 or not b.is_contiguous()):
                return None
            keep += [W, b]
            d.layer[i].W, d.layer[i].b = W.data_ptr(), (0 if b is None else b.data_ptr())
            d.layer[i].out_dim, d.layer[i].in_dim, d.layer[i].sigma_col = W.shape[0], W.shape[1], col
        d.n_layers, d.dim, d.n_wrapped = len(lins), self.dim, len(wrapped)
        d.act = _hip.ACT_CODES[net.activation_name]
        d.final_act = _hip.ACT_CODES[fa] if fa is not None else 0
        if self.dim > 128:
            return None
        if _hip.lib().sx_resnet_lds_bytes(d) > _hip.RESNET_LDS_BYTES:
            return None
        return d, keep, wrapped

    def _sigma_table(self, wrapped, n_calls, like, frozen: bool = False):
        """sx_spectral_sigma for `n_calls` hook calls of every wrapped layer (u / v advanced in place) -> (sigma [rows, n_wrapped],
        rows).  Eval mode (no layer training) or `frozen`: one row, no update (frozen: the plain `weight` stays too)."""
        if not wrapped:
            return None, 1
        training = not frozen and any(lin.training and hook.n_power_iterations > 0 for lin, hook in wrapped)
        rows = n_calls if training else 1
        job = _hip.sx_sn_job()
        for j, (lin, hook) in enumerate(wrapped):
            W, u, v = lin.weight_orig, lin.weight_u, lin.weight_v
            for tsr in (W, u, v):
                if tsr.dtype != torch.float32 or not tsr.is_contiguous():
                    raise TypeError('stribor_amd: spectral-norm tensors must be contiguous float32')
            job.layer[j].W, job.layer[j].u, job.layer[j].v = W.data_ptr(), u.data_ptr(), v.data_ptr()
            job.layer[j].out_dim, job.layer[j].in_dim = W.shape[0], W.shape[1]
            job.layer[j].n_power = hook.n_power_iterations if lin.training and not frozen else 0
            job.layer[j].eps = hook.eps
        job.n_layers = len(wrapped)
        sigma = torch.empty(rows, len(wrapped), dtype=torch.float32, device=like.device)
        _hip.call('sx_spectral_sigma', like, ctypes.byref(job), rows, sigma.data_ptr())
        if frozen:
            return sigma, rows
        # the plain `weight` attribute the reference's hook leaves behind: weight_orig / sigma of the last call
        for j, (lin, hook) in enumerate(wrapped):
            setattr(lin, hook.name, lin.weight_orig.detach() / sigma[rows - 1, j])
        return sigma, rows

    def _run_rows(self, x2, t2, iterations: int, inverse: bool, s=None, plan=None, sigma=None):
        """No-graph evaluation on [n, dim] fp32 rows: forward (inverse=False) or the `iterations`-step inverse.  The autograd ops
        pass s = time_net(t) as rows (then t2 is not read), their plan, and a sigma table they have already made."""
        n_calls = iterations if inverse else 1
        if inverse and iterations == 0:
            return x2.clone()
        if plan is None:
            plan = self._kernel_net()
        tn = self._time()
        tkind = None
        if tn is not None and plan is not None and s is None:
            tkind = _time_kind(tn)
            if tkind is not None:
                w = tn.scale if tkind in (1, 2, 3) else (tn.weight if tkind == 4 else None)
                if w is not None and w.numel() != self.dim * (tn.hidden_dim if tkind == 4 else 1):
                    tkind = None
            if tkind is not None and t2 is not None and t2.dim() == 2 and t2.shape[1] != 1:
                tkind = None
        if plan is None:
            return self._run_composed(x2, t2, iterations, inverse)
        d, keep, wrapped = plan
        n = x2.shape[0]
        sigma, rows = self._sigma_table(wrapped, n_calls, x2) if sigma is None else sigma
        out = torch.empty_like(x2)
        t_rows = s_rows = ta = tb = None
        kind, hidden = _hip.RESNET_TIME_NONE, 0
        if tn is not None:
            if tkind is None:
                kind = _hip.RESNET_TIME_ROWS
                s_rows = (self._s(t2, n, x2) if s is None else s.detach()).to(torch.float32).contiguous()
            else:
                kind = tkind
                t_rows = t2.reshape(n).to(torch.float32).contiguous()
                if tkind in (1, 2, 3):
                    ta = tn.scale.detach().reshape(-1).to(torch.float32).contiguous()
                elif tkind == 4:
                    ta = tn.get_scale().detach().to(torch.float32).contiguous()
                    tb = tn.shift.detach().to(torch.float32).contiguous()
                    hidden = tn.hidden_dim
        if n:
            _hip.call('sx_resnet_flow', x2, ctypes.byref(d), x2.data_ptr(), out.data_ptr(), n, _hip.ptr(t_rows), _hip.ptr(s_rows), kind,
                      _hip.ptr(ta), _hip.ptr(tb), hidden, _hip.ptr(sigma), rows, int(iterations), int(inverse))
        del keep
        return out

    def _run_composed(self, x2, t2, iterations: int, inverse: bool):
        """The composition fallback: the product MLP per evaluation (its torch layers, hooks included) and torch element-wise ops,
        the reference's loop and sigma schedule (iresnet.py:38-46, 80-90)."""
        s = self._s(t2, x2.shape[0], x2) if self._time() is not None else None
        if not inverse:
            g = self.net(x2)
            return x2 + (g if s is None else s * g)
        x = x2
        for _ in range(iterations):
            g = self.net(x)
            x = x2 - (g if s is None else s * g)
        return x

    def _composed_reference(self, x, t=None, iterations: int = 100, inverse: bool = True):
        """The composition fallback on any leading shape (tests and tools/bench_resnet_flow.py compare the kernel with it)."""
        x2, lead, t2 = self._rows(x, t)
        with torch.no_grad():
            return self._run_composed(x2, t2, iterations, inverse).reshape(*lead, self.dim)

    # ---- entry points -------------------------------------------------------------------------------------------------------
    def _rows(self, x, t):
        _hip.require_device(x, 'x')
        if x.dtype != torch.float32:
            raise TypeError(f'stribor_amd: IResNet takes float32 input (got {x.dtype})')
        x2, lead = flatten_rows(x)
        t2 = None
        if self._time() is not None:
            if t is None:
                raise TypeError('ContinuousIResNet needs t')
            t = t.to(device=x.device, dtype=torch.float32)
            tc = t.shape[-1] if t.dim() else 1
            t2 = t.expand(*lead, tc).reshape(-1, tc)
        return x2, lead, t2

    def _params(self):
        return [p for p in self.parameters()]

    def _call(self, x, t, iterations: int, inverse: bool):
        x2, lead, t2 = self._rows(x, t)
        if graph_wanted(self, x, t):
            plan = self._train_plan()
            self._last_grad_path = 'composed' if plan is None else 'kernel'
            if plan is not None:
                sr = None
                if self._time() is not None:
                    sr = self._s(t2, x2.shape[0], x2).to(torch.float32).contiguous()
                params = [p for p, _ in self._param_list()]
                if not inverse:
                    out = _ForwardFn.apply(self, x2, sr, *params)
                else:
                    out = _InverseFn.apply(self, x2, sr, int(iterations), *params)
                return out.reshape(*lead, self.dim)
            if not inverse:
                r = self._residual(x2, t2, frozen=False)
                return (x2 + r).reshape(*lead, self.dim)
            params = self._params()
            out = _InverseComposedFn.apply(self, x2, t2, int(iterations), *params)
            return out.reshape(*lead, self.dim)
        with torch.no_grad():
            y2 = self._run_rows(x2, None if t2 is None else t2.contiguous(), int(iterations), inverse)
        return y2.reshape(*lead, self.dim)

    def _inverse_rows(self, y2, t2, iterations):
        return self._run_rows(y2, None if t2 is None else t2.contiguous(), int(iterations), True)

    def log_det_jacobian(self, x, y=None, **kwargs):
        return NotImplementedError                            # iresnet.py:48-49, 95-96: returned, not raised


class IResNet(_IResNetBase):
    """Invertible ResNet y = x + g(x), g = spectral-normalised MLP (iresnet.py:9-49).

    ``inverse(y, iterations=100)`` runs exactly `iterations` fixed-point steps x <- y - g(x) from x = y (no early exit).  With an
    autograd graph, gradients reach x, weight_orig -- through sigma too -- and the biases, and ``inverse`` differentiates implicitly
    at the fixed point (exact up to convergence error; in training mode with the last iteration's sigma): on ``sx_resnet_flow_bwd``
    inside its coverage (``_ForwardFn`` / ``_InverseFn``), by composing torch ops outside it (``_InverseComposedFn``)."""

    def __init__(self, dim: int, hidden_dims: List[int], activation: str = 'ReLU', final_activation: str = None,
                 n_power_iterations: int = 5, **kwargs):
        super().__init__()
        self._make_net(dim, hidden_dims, activation, final_activation, n_power_iterations)

    def forward(self, x, **kwargs):
        return self._call(x, None, 1, False)

    def inverse(self, y, iterations=100, **kwargs):
        return self._call(y, None, iterations, True)


class ContinuousIResNet(_IResNetBase):
    """Continuous-time invertible ResNet y = x + time_net(t) * g(x) (iresnet.py:52-99); see ``IResNet``.  The time embeddings
    of net.time_net (TimeIdentity / Linear / Tanh / Log / Fourier[Bounded]) are evaluated inside the kernel; any other
    time net is called as a module and its output passed to the kernel."""

    def __init__(self, dim: int, hidden_dims: List[int], *, activation: str = 'ReLU', final_activation: str = None,
                 time_net: torch.nn.Module = None, n_power_iterations: int = 5, **kwargs):
        super().__init__()
        self._make_net(dim, hidden_dims, activation, final_activation, n_power_iterations)
        self.time_net = time_net

    def forward(self, x, t, **kwargs):
        return self._call(x, t, 1, False)

    def inverse(self, y, t, iterations=100, **kwargs):
        return self._call(y, t, iterations, True)
