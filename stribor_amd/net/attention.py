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

__all__ = ['attention', 'Attention', 'SelfAttention', 'InducedSelfAttention', 'self_attention_closed_form']


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

    def forward_twice_differentiable(self, query, key, value, mask=None, **kwargs):
        """The layer through plain torch ops (library GEMMs): differentiable to any order, where `forward`'s attention core and
        `batch_linear` are differentiable once.  For callers that differentiate a derivative (a CNF's divergence in training)."""
        q, k, v = (m.forward_twice_differentiable(t) for m, t in ((self.query, query), (self.key, key), (self.value, value)))
        y = _attention_composed(q, k, v, self.n_heads, self.mask_diagonal, None if mask is None else mask.to(q.dtype))
        return F.linear(y, self.proj.weight, self.proj.bias)


class SelfAttention(Attention):
    """Attention of a set with itself (attention.py:101-122): forward(x, mask)."""

    def __init__(self, in_dim: int, hidden_dim: List[int], out_dim: int, n_heads: int = 1, mask_diagonal: bool = False, **kwargs):
        super().__init__(in_dim, hidden_dim, out_dim, n_heads, mask_diagonal)

    def forward(self, x, mask=None, **kwargs):
        return super().forward(x, x, x, mask=mask)

    def forward_twice_differentiable(self, x, mask=None, **kwargs):
        return super().forward_twice_differentiable(x, x, x, mask=mask)


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


def _act_prime(layer: nn.Module, z: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """act'(z) of an elementwise activation `layer` with a = layer(z): closed forms for the activations the CNF kernels know (torch's
    default parameters are read off the layer), one elementwise reverse pass for any other."""
    kind = type(layer)
    if kind is nn.Identity:
        return torch.ones_like(z)
    if kind is nn.Tanh:
        return 1 - a * a
    if kind is nn.ReLU:
        return (z > 0).to(z.dtype)
    if kind is nn.Sigmoid:
        return a * (1 - a)
    if kind is nn.ELU:
        return torch.where(z > 0, torch.ones_like(z), a + layer.alpha)
    if kind is nn.Softplus:
        return torch.where(z * layer.beta > layer.threshold, torch.ones_like(z), torch.sigmoid(z * layer.beta))
    if kind is nn.LeakyReLU:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, layer.negative_slope))
    with torch.enable_grad():
        zz = z.detach().requires_grad_(True)
        return torch.autograd.grad(layer(zz).sum(), zz)[0]


def self_attention_closed_form(net, t, x, latent=None, want_div: bool = True, dtype=None):
    """f = net(t, x, latent) of a ``DiffeqSelfAttention`` (or its ``SelfAttention`` over the columns [t, x, latent]) on sets (..., N,
    dim), and -- `want_div` -- div[..., i, d] = d f_i[d] / d x_i[d] WITHOUT autograd: what ``divergence_exact_for_sets`` gives with N *
    dim reverse passes, and what ``sx_cnf_attn_flow`` integrates (DESIGN.md "CNF on sets with attention").  Per coordinate d a forward
    tangent of x_i[d] runs through element i's own embeddings (qd, kd, vd); per head, with s = scale q k^T, p = safe_softmax(s):
        sd_ij = scale qd_i . k_j + [i == j] scale q_i . kd_i            (the second term is absent under mask_diagonal: p_ii = 0)
        od_i  = sum_j p_ij (sd_ij - sum_m p_im sd_im) v_j + p_ii vd_i
        div[i, d] = proj.weight[d, head columns] . od_i, summed over the heads.
    Plain torch on any device in `dtype` (default: x's).  -> (dy, div | None)."""
    att = net.net if isinstance(getattr(net, 'net', None), Attention) else net
    dtype = dtype or x.dtype
    x = x.to(dtype)
    D, H = x.shape[-1], att.n_heads
    cols = [torch.ones_like(x[..., :1]) * torch.as_tensor(t).reshape(-1)[0].to(x), x]
    if latent is not None:
        cols.append(latent.to(device=x.device, dtype=dtype).expand(*x.shape[:-1], latent.shape[-1]))
    u = torch.cat(cols, -1)

    def embed(mlp):
        h, hd = u, None                                       # hd [..., N, D, width]: the tangent of x_i[d] through element i
        for layer in mlp.net:
            if isinstance(layer, nn.Linear):
                W = layer.weight.detach().to(dtype)
                b = None if layer.bias is None else layer.bias.detach().to(dtype)
                if want_div:
                    hd = W[:, 1:1 + D].t() if hd is None else hd @ W.t()
                h = F.linear(h, W, b)
            else:
                a = layer(h)
                if want_div:
                    hd = hd * _act_prime(layer, h, a).unsqueeze(-2)
                h = a
        return h, hd
    (q, qd), (k, kd), (v, vd) = embed(att.query), embed(att.key), embed(att.value)
    E = q.shape[-1]
    dh = E // H
    N = x.shape[-2]
    scale = (1 / dh) ** 0.5
    heads = lambda z: z.reshape(*z.shape[:-1], H, dh)
    qh, kh, vh = heads(q), heads(k), heads(v)
    s = torch.einsum('...ihe,...jhe->...hij', qh, kh) * scale
    eye = torch.eye(N, dtype=torch.bool, device=x.device)
    if att.mask_diagonal:
        s = s.masked_fill(eye, -float('inf'))
    p = safe_softmax(s, -1)
    P = att.proj.weight.detach().to(dtype)
    o = torch.einsum('...hij,...jhe->...ihe', p, vh)
    dy = F.linear(o.reshape(*x.shape[:-1], E), P, None if att.proj.bias is None else att.proj.bias.detach().to(dtype))
    if not want_div:
        return dy, None
    expand = lambda z: heads(z.expand(*x.shape[:-1], D, E))                          # [..., N, D, H, dh]
    qdh, kdh, vdh = expand(qd), expand(kd), expand(vd)
    sd = torch.einsum('...idhe,...jhe->...hidj', qdh, kh) * scale
    if not att.mask_diagonal:
        own = torch.einsum('...ihe,...idhe->...hid', qh, kdh) * scale
        sd = sd + own.unsqueeze(-1) * eye.to(dtype).unsqueeze(-2)                     # [..., H, N, D, N]: only at j == i
    pe = p.unsqueeze(-2)                                                             # [..., H, N, 1, N]
    w = pe * (sd - (pe * sd).sum(-1, keepdim=True))
    pii = torch.diagonal(p, dim1=-2, dim2=-1)                                        # [..., H, N]
    od = torch.einsum('...hidj,...jhe->...idhe', w, vh) + pii.transpose(-1, -2)[..., None, :, None] * vdh
    div = torch.einsum('...ide,de->...id', od.reshape(*x.shape[:-1], D, E), P)
    return dy, div
