"""Permutation-equivariant layers over sets of shape (..., N, dim) (reference: stribor/net/equivariant.py:6-93).

Same constructors, ``state_dict`` keys (``layers.<i>.l1.weight``, ``layers.<i>.l2.weight``, ...) and RNG draws: per layer ``l1`` then
``l2``, both default-initialised ``nn.Linear``.

``EquivariantNet.forward`` on a ROCm tensor is ONE launch of the HIP kernel ``sx_equivariant_fwd`` (the hidden activations never
reach HBM) and, under a graph, ``sx_equivariant_bwd`` (dx and every parameter gradient; no atomics, bit-reproducible; the mask gets
no gradient) -- when ``kernel_plan`` covers the call.  Everything else -- CPU tensors, shapes outside the
coverage, subclasses, empty batches -- runs the reference's op sequence, which stays available as ``forward_twice_differentiable``:
the composition path of ``ContinuousTransform`` differentiates the divergence of this net and calls that (``DiffeqConcat``).  On its
kernel path ``ContinuousTransform`` calls neither: ``sx_cnf_set_flow`` consumes the weights directly.
"""
import math
from typing import List

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _hip
from . import cover

__all__ = ['EquivariantLayer', 'EquivariantNet', 'equivariant_backward_closed_form']


class EquivariantLayer(nn.Module):
    """y_i = l1(x_i) + l2(sum_j x_j) / N -- with ``mask`` (..., N, 1): masked elements give 0 and N is the number kept
    (equivariant.py:33-43; ``l2``'s bias is divided too)."""

    def __init__(self, in_dim: int, out_dim: int, **kwargs):
        super().__init__()
        self.l1 = nn.Linear(in_dim, out_dim)
        self.l2 = nn.Linear(in_dim, out_dim)

    def forward(self, x, mask=None, **kwargs):
        y1 = self.l1(x)
        y2 = self.l2(x.sum(-2, keepdim=True))
        if mask is not None:
            mask = mask[..., 0, None]
            y1 = y1 * mask
            y2 = y2 * mask / mask.sum(-2, keepdim=True)
        else:
            y2 = y2 / x.shape[-2]
        return y1 + y2


def _descriptor(params, dims, act: int, final_act: int, set_size: int):
    d = _hip.sx_equivariant_net()
    for l in range(len(dims) - 1):
        d.A[l], d.a[l], d.B[l], d.b[l] = (t.data_ptr() for t in params[4 * l:4 * l + 4])
        d.out_dim[l] = dims[l + 1]
    d.n_layers, d.in_dim, d.act, d.final_act, d.set_size = len(dims) - 1, dims[0], act, final_act, set_size
    return d


class _EquivariantCore(torch.autograd.Function):
    """y [rows, out] = the net over x [rows, in] (unit column stride, any row stride), rows = sets x N, with an optional per-row mask
    column: sx_equivariant_fwd, and sx_equivariant_bwd for dx and the parameter gradients.  Nothing but x and the mask is saved."""

    @staticmethod
    def forward(ctx, x2, m2, cfg, *params):
        dims, act, final_act, N = cfg
        rows = x2.shape[0]
        y = torch.empty(rows, dims[-1], dtype=torch.float32, device=x2.device)
        d = _descriptor(params, dims, act, final_act, N)
        _hip.call('sx_equivariant_fwd', x2, _hip.C.byref(d), x2.data_ptr(), x2.stride(0), _hip.ptr(m2), 0 if m2 is None else m2.stride(0),
                  y.data_ptr(), rows)
        ctx.save_for_backward(x2, m2, *params)
        ctx.cfg = cfg
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x2, m2, *params = ctx.saved_tensors
        dims, act, final_act, N = ctx.cfg
        rows = x2.shape[0]
        need = ctx.needs_input_grad
        gy = gy.to(torch.float32).contiguous()
        d = _descriptor(params, dims, act, final_act, N)
        dx = torch.empty(rows, dims[0], dtype=torch.float32, device=x2.device) if need[0] else None
        grads = [torch.empty_like(p) if need[3 + i] else None for i, p in enumerate(params)]
        g = _hip.sx_equivariant_grads()
        for l in range(len(dims) - 1):
            g.dA[l], g.da[l], g.dB[l], g.db[l] = (_hip.ptr(t) for t in grads[4 * l:4 * l + 4])
        partial = None
        if any(t is not None for t in grads):
            partial = _hip.scratch(x2.device, _hip.lib().sx_equivariant_bwd_partial_floats(_hip.C.byref(d), rows))
        if dx is not None or partial is not None:
            _hip.call('sx_equivariant_bwd', x2, _hip.C.byref(d), x2.data_ptr(), x2.stride(0), _hip.ptr(m2), 0 if m2 is None else m2.stride(0),
                      gy.data_ptr(), _hip.ptr(dx), _hip.ptr(partial), _hip.C.byref(g), rows)
        return (dx, None, None, *grads)


class EquivariantNet(nn.Module):
    """``EquivariantNet(in_dim, hidden_dims, out_dim, activation='Tanh', final_activation=None)``: ``net.MLP``'s arguments with
    ``EquivariantLayer`` in place of ``nn.Linear`` (equivariant.py:45-93).  ``_last_path`` is ``'kernel'`` or ``'composed'`` after
    each call of ``forward``.

    >>> net = stribor_amd.net.EquivariantNet(2, [64, 64], 4)
    """
    _last_path = None

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, activation: str = 'Tanh', final_activation: str = None,
                 **kwargs):
        super().__init__()
        self.activation = getattr(nn, activation)()
        self.final_activation = getattr(nn, final_activation)() if final_activation else nn.Identity()
        dims = [in_dim] + list(hidden_dims) + [out_dim]
        self.layers = nn.ModuleList([EquivariantLayer(a, b) for a, b in zip(dims[:-1], dims[1:])])

    def kernel_plan(self, shape, graph: bool, device):
        """(parameters, dims, act code, final act code) when the HIP kernel covers a call on an input of `shape` with the parameters on
        `device` -- and, with `graph`, its backward too -- else None.  Host code: shapes and the library's LDS sizes only.  Covered:
        exactly this class over ``EquivariantLayer``s of two biased ``nn.Linear``s, one or two hidden layers, both activations among
        the seven with an in-kernel derivative at torch's defaults, fp32 contiguous parameters, and a shape inside
        ``sx_equivariant_lds_bytes``'s coverage (the planner's answer is that function's)."""
        if type(self) is not EquivariantNet or len(self.layers) not in (2, 3) or len(shape) < 2:
            return None
        act, fact = type(self.activation).__name__, type(self.final_activation).__name__
        if not (cover.kernel_activation(act, [self.activation]) and cover.kernel_activation(fact, [self.final_activation])):
            return None
        params, dims = [], [shape[-1]]
        for layer in self.layers:
            if type(layer) is not EquivariantLayer or type(layer.l1) is not nn.Linear or type(layer.l2) is not nn.Linear:
                return None
            if layer.l1.bias is None or layer.l2.bias is None or layer.l1.weight.shape != layer.l2.weight.shape:
                return None
            if layer.l1.in_features != dims[-1]:
                return None
            params += [layer.l1.weight, layer.l1.bias, layer.l2.weight, layer.l2.bias]
            dims.append(layer.l1.out_features)
        if not cover.kernel_tensors(params, device) or math.prod(shape) == 0:
            return None
        plan = (params, tuple(dims), _hip.ACT_CODES[act], _hip.ACT_CODES[fact])
        d = _descriptor(params, dims, plan[2], plan[3], shape[-2])
        lib = _hip.lib()
        if lib.sx_equivariant_lds_bytes(_hip.C.byref(d), 0) == 0 or (graph and lib.sx_equivariant_lds_bytes(_hip.C.byref(d), 1) == 0):
            return None
        return plan

    def forward(self, x, mask=None, **kwargs):
        plan = None
        if x.is_cuda and x.is_floating_point() and (mask is None or mask.is_cuda):
            graph = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
            plan = self.kernel_plan(x.shape, graph, x.device)
        if plan is None:
            self._last_path = 'composed'
            return self.forward_twice_differentiable(x, mask=mask)
        if mask is not None and mask.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError('stribor_amd.net.EquivariantNet: the mask gets no gradient (pass mask.detach())')
        params, dims, act, fact = plan
        lead, N = x.shape[:-2], x.shape[-2]
        x2 = x.to(torch.float32).reshape(-1, dims[0])
        if x2.stride(1) != 1 or x2.stride(0) < dims[0] or x2.data_ptr() % 4:
            x2 = x2.contiguous()
        m2 = None
        if mask is not None:
            m2 = mask.detach().to(torch.float32)
            m2 = m2.expand(*lead, N, m2.shape[-1]).reshape(-1, m2.shape[-1])[:, 0]          # column 0, read in place
            if m2.stride(0) < 1 or m2.data_ptr() % 4:
                m2 = m2.contiguous()
        y = _EquivariantCore.apply(x2, m2, (dims, act, fact, N), *params)
        self._last_path = 'kernel'
        return y.reshape(*lead, N, dims[-1])

    def forward_twice_differentiable(self, x, mask=None, **kwargs):
        """The net through plain torch ops -- the reference's op sequence, on any device: differentiable to any order, where
        ``forward``'s kernel is differentiable once.  For callers that differentiate a derivative (a CNF's divergence)."""
        for layer in self.layers[:-1]:
            x = self.activation(layer(x, mask=mask))
        return self.final_activation(self.layers[-1](x, mask=mask))


def equivariant_backward_closed_form(layers, activation, final_activation, x, mask, gy):
    """The backward of ``EquivariantNet`` in torch ops, any dtype and device: the statement ``sx_equivariant_bwd`` is written from
    (DESIGN.md section 4.16).  `layers`: ``EquivariantLayer``s or (A, a, B, b) tuples; `activation` / `final_activation`: names or
    modules among the seven of ``cover.ACTS``; x (..., N, in); mask (..., N, k) or None (it gets no gradient); gy = dloss/dy.
    -> (dx, [(dA, da, dB, db) per layer]).  With e_l = dloss/dz_l, m_i = mask[..., i, 0] (1 without a mask), w_i = m_i / sum_j m_j
    (1 / N without a mask) and S_{l-1} the sum of h_{l-1} over the WHOLE set: dA_l = sum_i m_i e_l,i h_{l-1,i}^T, da_l = sum_i m_i e_l,i,
    r_l = sum_{i in set} w_i e_l,i, dB_l = sum_sets r_l S_{l-1}^T, db_l = sum_sets r_l, dh_{l-1,i} = A_l^T (m_i e_l,i) + B_l^T r_l,
    e_{l-1} = act'(h_{l-1}) dh_{l-1} with act' taken from the activation's output."""
    name = lambda a: 'Identity' if a is None else a if isinstance(a, str) else type(a).__name__
    act, dact = cover.ACTS[name(activation)][:2]
    fact, dfact = cover.ACTS[name(final_activation)][:2]
    ws = [tuple(t.detach().to(x.dtype) for t in ((l.l1.weight, l.l1.bias, l.l2.weight, l.l2.bias) if isinstance(l, nn.Module) else l))
          for l in layers]
    N = x.shape[-2]
    m = None if mask is None else mask[..., 0, None].to(x.dtype)
    c = None if m is None else m.sum(-2, keepdim=True)
    hs, Ss, h = [], [], x
    for i, (A, a, B, b) in enumerate(ws):
        S = h.sum(-2, keepdim=True)
        hs.append(h)
        Ss.append(S)
        y1, y2 = h @ A.t() + a, S @ B.t() + b
        z = y1 + y2 / N if m is None else y1 * m + y2 * m / c
        h = act(z) if i + 1 < len(ws) else fact(z)
    e = dfact(h) * gy
    grads = [None] * len(ws)
    for i in reversed(range(len(ws))):
        A, a, B, b = ws[i]
        me = e if m is None else e * m
        r = (e / N if m is None else e * (m / c)).sum(-2, keepdim=True)
        flat = lambda t: t.reshape(-1, t.shape[-1])
        grads[i] = (flat(me).t() @ flat(hs[i]), flat(me).sum(0), flat(r).t() @ flat(Ss[i]), flat(r).sum(0))
        dh = me @ A + r @ B
        if i > 0:
            e = dact(hs[i]) * dh
    return dh, grads
