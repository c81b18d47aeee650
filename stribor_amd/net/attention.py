"""Attention nets (reference: stribor/net/attention.py:8-147): ``attention``, ``Attention``, ``SelfAttention`` and
``InducedSelfAttention``, the set-aware conditioners of a ``Coupling(..., set_data=True)``.

Same constructors, same ``state_dict`` keys (``key.net.0.weight`` ..., ``proj.*``, ``points``, ``att1.*``, ``att2.*``) and the same
construction order, hence the same RNG draws: key, query and value embeddings (the product ``net.MLP``), then ``proj``; ``att1``,
``att2``, then ``points``.

The multi-head attention itself (attention.py:26-49 with safe_softmax) is the HIP core ``sx_attention_fwd`` -- ONE launch,
flash-style: the [..., H, Nq, Nk] score tensor never reaches HBM -- and, under a graph, ``sx_attention_bwd`` (dq, dk, dv; no atomics,
bit-reproducible).  Its arithmetic is exact fp32 (v_mfma_f32_32x32x2_f32) whatever ``set_gemm_precision`` says.  Heads wider than
128 features run a torch composition with the same semantics.  When the three embeddings are single Linear layers and see the same
input (``SelfAttention``), they run as ONE GEMM over the concatenated [3E, in] weight, and the core reads q, k and v out of the
[rows, 3E] result through its row stride, without copies.  The mask gets no gradient.
"""
import math
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _hip
from ..fused import StructureTracked
from ..util.safe_softmax import safe_softmax
from .mlp import MLP, _Linear, batch_linear

__all__ = ['attention', 'Attention', 'SelfAttention', 'InducedSelfAttention']


def _core_args(q, k, v, mask2, n_heads: int, mask_diagonal: bool, out_mask: bool):
    a = _hip.sx_attention_args()
    a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    a.q_bs, a.q_rs = q.stride(0), q.stride(1)
    a.k_bs, a.k_rs = k.stride(0), k.stride(1)
    a.v_bs, a.v_rs = v.stride(0), v.stride(1)
    a.mask = None if mask2 is None else mask2.data_ptr()
    a.mask_bs = 0 if mask2 is None else mask2.stride(0)
    a.R, a.Nq, a.Nk, a.E, a.n_heads = q.shape[0], q.shape[1], k.shape[1], q.shape[2], n_heads
    a.mask_diagonal, a.out_mask = int(bool(mask_diagonal)), int(bool(out_mask))
    return a


def _empty(R: int, Nq: int, Nk: int) -> bool:
    return R == 0 or Nq == 0 or Nk == 0


class AttentionCore(torch.autograd.Function):
    """y [R, Nq, E] = multi-head attention of q [R, Nq, E], k / v [R, Nk, E] (unit column stride, any batch / row stride) with an
    optional per-key mask [R, Nk]: sx_attention_fwd, and sx_attention_bwd for dq, dk, dv (the mask gets no gradient)."""

    @staticmethod
    def forward(ctx, q, k, v, mask2, n_heads: int, mask_diagonal: bool, out_mask: bool):
        R, Nq, E = q.shape
        Nk = k.shape[1]
        alloc = torch.zeros if _empty(R, Nq, Nk) else torch.empty        # (the core writes every row)
        y = alloc(R, Nq, E, dtype=torch.float32, device=q.device)
        lse = torch.empty(R, n_heads, Nq, dtype=torch.float32, device=q.device)
        if not _empty(R, Nq, Nk):                   # (no key: every query is fully masked, its output is 0)
            a = _core_args(q, k, v, mask2, n_heads, mask_diagonal, out_mask)
            _hip.call('sx_attention_fwd', q, _hip.C.byref(a), y.data_ptr(), lse.data_ptr())
        ctx.save_for_backward(q, k, v, mask2, y, lse)
        ctx.cfg = (n_heads, mask_diagonal, out_mask)
        return y

    @staticmethod
    def backward(ctx, gy):
        q, k, v, mask2, y, lse = ctx.saved_tensors
        n_heads, mask_diagonal, out_mask = ctx.cfg
        R, Nq, E = q.shape
        Nk = k.shape[1]
        alloc = torch.zeros if _empty(R, Nq, Nk) else torch.empty        # (the two passes write every row)
        dq = alloc(R, Nq, E, dtype=torch.float32, device=q.device)
        dk = alloc(R, Nk, E, dtype=torch.float32, device=q.device)
        dv = alloc(R, Nk, E, dtype=torch.float32, device=q.device)
        if not _empty(R, Nq, Nk):
            gy = gy.to(torch.float32).contiguous()
            delta = torch.empty(R, n_heads, Nq, dtype=torch.float32, device=q.device)
            a = _core_args(q, k, v, mask2, n_heads, mask_diagonal, out_mask)
            _hip.call('sx_attention_bwd', q, _hip.C.byref(a), y.data_ptr(), gy.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                      dk.data_ptr(), dv.data_ptr(), delta.data_ptr())
        return dq, dk, dv, None, None, None, None


def _attention_composed(query, key, value, n_heads: int, mask_diagonal: bool, mask):
    """attention.py:26-49 as torch ops on the device (heads wider than the core's 128 features; tests and benchmarks)."""
    *lq, Nq, E = query.shape
    *lk, Nk, _ = key.shape
    dh = E // n_heads

    def heads(t, lead, n):
        return t.reshape(*lead, n, n_heads, dh).transpose(-2, -3)
    qh, kh, vh = heads(query, lq, Nq), heads(key, lk, Nk), heads(value, lk, Nk)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * (1 / dh) ** 0.5
    if mask_diagonal:
        s = s.masked_fill(torch.eye(Nk, dtype=torch.bool, device=s.device), -float('inf'))
    if mask is not None:
        drop = (mask != 1).transpose(-1, -2).unsqueeze(-3)            # (..., 1, 1, Nk)
        s = s.masked_fill(drop, -float('inf'))
    y = torch.matmul(safe_softmax(s, -1), vh).transpose(-2, -3).reshape(*lq, Nq, E)
    if mask is not None and Nq == mask.shape[-2]:
        y = y * mask
    return y


def _rows3(t: torch.Tensor, n: int, e: int) -> torch.Tensor:
    t = t.to(torch.float32).reshape(math.prod(t.shape[:-2]), n, e)
    return t if t.stride(2) == 1 else t.contiguous()


def attention(query, key, value, n_heads: int = 1, mask_diagonal: bool = False, mask=None):
    """Multi-head attention with optional masking (attention.py:8-49): query (..., Nq, E), key / value (..., Nk, E), mask
    (..., Nk, 1).  A key is ignored iff its mask is not 1; a query whose keys are all ignored gets 0.  When Nq == Nk the output
    rows are multiplied by the mask.  fp32 result; one launch of the HIP core for heads of up to 128 features."""
    for t, name in ((query, 'query'), (key, 'key'), (value, 'value')):
        _hip.require_device(t, f'attention {name}')
    if mask is not None:
        _hip.require_device(mask, 'attention mask')
        if mask.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError('stribor_amd.net.attention: the mask gets no gradient (pass mask.detach())')
    E = value.shape[-1]
    Nq, Nk = query.shape[-2], value.shape[-2]
    if E % n_heads != 0 or query.shape[-1] != E or key.shape != value.shape:
        raise RuntimeError(f'attention: cannot split {tuple(query.shape)} / {tuple(key.shape)} / {tuple(value.shape)} into '
                           f'{n_heads} heads')
    if mask_diagonal and Nq != Nk:
        raise RuntimeError(f'attention: mask_diagonal needs as many queries as keys (got {Nq} and {Nk})')
    if query.shape[:-2] != value.shape[:-2]:
        raise RuntimeError(f'attention: query and key / value leading shapes differ ({tuple(query.shape)}, {tuple(value.shape)})')
    if E // n_heads > _hip.ATTENTION_MAX_HEAD_DIM:
        f32 = lambda t: None if t is None else t.to(torch.float32)
        return _attention_composed(f32(query), f32(key), f32(value), n_heads, mask_diagonal, f32(mask))
    lead = query.shape[:-2]
    q, k, v = _rows3(query, Nq, E), _rows3(key, Nk, E), _rows3(value, Nk, E)
    mask2 = None
    out_mask = False
    if mask is not None:
        out_mask = Nq == mask.shape[-2]
        mask2 = mask.detach().to(torch.float32).expand(*lead, Nk, 1).reshape(math.prod(lead), Nk)
        if mask2.stride(1) != 1:
            mask2 = mask2.contiguous()
    y = AttentionCore.apply(q, k, v, mask2, n_heads, bool(mask_diagonal), out_mask)
    return y.reshape(*lead, Nq, E)


def _embed(net: MLP, x: torch.Tensor) -> torch.Tensor:
    """net(x); an input broadcast over its leading dimensions (InducedSelfAttention's inducing points) is embedded once."""
    if x.dim() > 2 and all(s == 0 for s in x.stride()[:-2]):
        return net(x[(0,) * (x.dim() - 2)]).expand(*x.shape[:-1], net.out_dim)
    return net(x)


def _wants_graph(x: torch.Tensor, params) -> bool:
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))


class Attention(StructureTracked, nn.Module):
    """Attention layer (attention.py:51-98): embeddings query / key / value = net.MLP(in_dim, hidden_dims[:-1], hidden_dims[-1]),
    multi-head attention over them, then proj = Linear(hidden_dims[-1], out_dim)."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, n_heads: int = 1, mask_diagonal: bool = False, **kwargs):
        super().__init__()
        self.mask_diagonal = mask_diagonal
        self.n_heads = n_heads
        self.key = MLP(in_dim, hidden_dims[:-1], hidden_dims[-1])
        self.query = MLP(in_dim, hidden_dims[:-1], hidden_dims[-1])
        self.value = MLP(in_dim, hidden_dims[:-1], hidden_dims[-1])
        self.proj = _Linear(hidden_dims[-1], out_dim)
        self._packed = None            # ((data_ptr, _version) of the six tensors, device) -> concatenated weight / bias

    def _single_linears(self):
        """The (weight, bias) of the query, key and value embeddings when each is one plain Linear layer, else None."""
        out = []
        for m in (self.query, self.key, self.value):
            ls = m.linears()
            if len(ls) != 1 or m._wrapped or m.final_activation_name is not None or ls[0][1] is None:
                return None
            out.append(ls[0])
        return out

    def _packed_qkv(self, lin, graph: bool):
        """[3E, in] weight and [3E] bias of the query | key | value embeddings: differentiable torch.cat under a graph, else
        cached per weight version."""
        ts = [t for wb in lin for t in wb]
        if graph:
            return torch.cat([w for w, _ in lin]), torch.cat([b for _, b in lin])
        key = (tuple((t.data_ptr(), t._version) for t in ts), str(ts[0].device))
        if self._packed is None or self._packed[0] != key:
            with torch.no_grad():
                self._packed = (key, torch.cat([w for w, _ in lin]).contiguous(), torch.cat([b for _, b in lin]).contiguous())
        return self._packed[1], self._packed[2]

    def _embed_all(self, query, key, value):
        lin = self._single_linears()
        if lin is None or not (query is key and key is value):
            return _embed(self.query, query), _embed(self.key, key), _embed(self.value, value)
        _hip.require_device(query, 'Attention input')
        E = lin[0][0].shape[0]
        x2 = query.reshape(-1, query.shape[-1]).to(torch.float32)
        graph = _wants_graph(query, [t for wb in lin for t in wb])
        W, b = self._packed_qkv(lin, graph)
        qkv = batch_linear(x2.contiguous(), W, b) if graph else F.linear(x2, W, b)      # ONE GEMM for the three embeddings
        lead = query.shape[:-1]
        return tuple(qkv[:, i * E:(i + 1) * E].reshape(*lead, E) for i in range(3))

    def _project(self, y: torch.Tensor) -> torch.Tensor:
        y2 = y.reshape(-1, y.shape[-1])
        W, b = self.proj.weight, self.proj.bias
        out = batch_linear(y2, W, b) if _wants_graph(y2, [W, b]) else F.linear(y2, W, b)
        return out.reshape(*y.shape[:-1], W.shape[0])

    def forward(self, query, key, value, mask=None, **kwargs):
        q, k, v = self._embed_all(query, key, value)
        return self._project(attention(q, k, v, self.n_heads, self.mask_diagonal, mask))


class SelfAttention(Attention):
    """Attention of a set with itself (attention.py:101-122): forward(x, mask)."""

    def __init__(self, in_dim: int, hidden_dim: List[int], out_dim: int, n_heads: int = 1, mask_diagonal: bool = False, **kwargs):
        super().__init__(in_dim, hidden_dim, out_dim, n_heads, mask_diagonal)

    def forward(self, x, mask=None, **kwargs):
        return super().forward(x, x, x, mask=mask)


class InducedSelfAttention(StructureTracked, nn.Module):
    """Induced self attention through n_points learned inducing points (attention.py:125-147): att1 attends from the points to
    the set (with the set's mask), att2 from the (masked) set to att1's output."""

    def __init__(self, in_dim: int, hidden_dim: List[int], out_dim: int, n_heads: int = 1, n_points: int = 32, **kwargs):
        super().__init__()
        self.att1 = Attention(in_dim, hidden_dim, in_dim, n_heads)
        self.att2 = Attention(in_dim, hidden_dim, out_dim, n_heads)
        self.points = nn.Parameter(torch.empty(n_points, in_dim).uniform_(-1., 1.))

    def forward(self, x, mask=None, **kwargs):
        h = self.points.expand(*x.shape[:-2], *self.points.shape)
        h = self.att1(h, x, x, mask=mask, **kwargs)
        return self.att2(x * (1 if mask is None else mask), h, h, **kwargs)
