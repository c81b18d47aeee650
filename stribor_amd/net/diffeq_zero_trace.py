"""Zero-trace differential-equation net (reference: stribor/net/diffeq_zero_trace.py:14-56): for ``divergence='exact'``.

``DiffeqZeroTraceMLP`` is the sum of two MADEs in the natural ordering, one of them reversed: output i of the first depends on the
inputs before i, of the second on the inputs after i, so together on every input but x_i -- the Jacobian is hollow and its trace 0.
Same constructor and ``state_dict`` keys (``net1.net.0.{weight,bias,mask}``, ``net2...``); ``net1`` is built (and draws) first.

``DiffeqZeroTraceDeepSet`` (diffeq_zero_trace.py:59-176) is the set instance over (..., N, dim): per element a MADE of its own
coordinates plus, the same for every dimension, a pooling of the OTHER elements' embeddings ``set_emb(t, x_j)`` -- the exclusive
sum / mean / max below.  Output (i, d) depends neither on x_i[d] (the MADE) nor on any coordinate of x_i (the pooling), so the
diagonal blocks d y[i, d, :] / d x[i, d] vanish.  Keys ``elementwise.net.<i>.{weight,bias,mask}``,
``interaction.set_emb.net.net.<i>.{weight,bias}``; the MADE is built (and draws) first.

``DiffeqZeroTraceAttention`` (diffeq_zero_trace.py:179-227) is the attention instance over (..., N, dim): per dimension d a query from
a MADE of the element's own coordinates (it does not depend on x_i[d]) attends, diagonal masked, to keys and values of the OTHER
elements, and a Linear projects the result to out_dim / dim slots.  Keys ``q.net.<i>.{weight,bias,mask}``, ``k.net.<i>.*``,
``v.net.<i>.*``, ``proj.net.0.*``; construction order q, k, v, proj.
"""
from typing import List, Optional

import torch
import torch.nn as nn

from .attention import attention
from .diffeq import DiffeqMLP, DiffeqNet
from .made import MADE
from .mlp import MLP

__all__ = ['DiffeqZeroTraceMLP', 'DiffeqZeroTraceDeepSet', 'DiffeqZeroTraceAttention', 'ZeroTraceEquivariantEncoder', 'exclusive_sum_pooling',
           'exclusive_mean_pooling', 'exclusive_max_pooling']


class DiffeqZeroTraceMLP(DiffeqNet):
    """``DiffeqZeroTraceMLP(dim, hidden_dims, k * dim)``: dx/dt with an exactly zero divergence; ignores t.

    forward(t, x) -> y [..., k * dim] (dimension-major: the k values of dimension i are columns i * k .. i * k + k - 1), and with
    ``return_log_det_jac`` (the default) the Jacobian diagonal beside it: zeros like x."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, return_log_det_jac: Optional[bool] = True, **kwargs):
        super().__init__()
        self.return_log_det_jac = return_log_det_jac
        self.net1 = MADE(in_dim, hidden_dims, out_dim, natural_ordering=True, reverse_ordering=False, return_per_dim=True)
        self.net2 = MADE(in_dim, hidden_dims, out_dim, natural_ordering=True, reverse_ordering=True, return_per_dim=True)

    def forward(self, t, x, **kwargs):
        y = self.net1(x, **kwargs) + self.net2(x, **kwargs)
        y = y.reshape(*y.shape[:-2], -1)
        return (y, torch.zeros_like(x)) if self.return_log_det_jac else y


def exclusive_sum_pooling(x, mask):
    """x [..., N, D] -> per element the sum over the OTHER elements of its set."""
    return x.sum(-2, keepdim=True) - x


def exclusive_mean_pooling(x, mask):
    """The exclusive sum over max(N - 1, 1), N = mask.sum(-2).  The divisor is the reference's expression: ``torch.max(...)[0]`` is
    the FIRST set's count, which is every set's count whenever no mask was given."""
    emb = exclusive_sum_pooling(x, mask)
    N = mask.sum(-2, keepdim=True)
    return emb / torch.max(N - 1, torch.ones_like(N))[0]


def exclusive_max_pooling(x, mask):
    """Per column the largest value among the OTHER elements: with first >= second the two largest values over the set (duplicates
    count), an element that holds `first` gets `second`.  A set of one element pools to 0."""
    if x.shape[-2] == 1:
        return torch.zeros_like(x)
    first, second = torch.topk(x, 2, dim=-2).values.chunk(2, dim=-2)
    indicator = (x == first).float()
    return (1 - indicator) * first + indicator * second


class ZeroTraceEquivariantEncoder(nn.Module):
    """forward(t, x [..., N, D], mask) -> [..., N, in_dim, out_dim]: ``set_emb = DiffeqMLP(in_dim + 1, hidden_dims, out_dim)`` on
    [t, x_j], pooled over the other elements ('mean' | 'max' | 'sum'), repeated for every dimension.  The default mask is built on
    x's device and dtype (the reference builds it on the CPU: DESIGN.md 4.11)."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, pooling: str, **kwargs):
        super().__init__()
        self.pooling = pooling
        self.in_dim = in_dim
        self.set_emb = DiffeqMLP(in_dim + 1, hidden_dims, out_dim)

    def forward(self, t, x, mask=None, **kwargs):
        if mask is None:
            mask = torch.ones(*x.shape[:-1], 1, device=x.device, dtype=x.dtype)
        else:
            mask = mask[..., 0, None]
        x = self.set_emb(t, x) * mask
        if self.pooling == 'mean':
            y = exclusive_mean_pooling(x, mask)
        elif self.pooling == 'max':
            y = exclusive_max_pooling(x, mask)
        elif self.pooling == 'sum':
            y = exclusive_sum_pooling(x, mask)
        return y.unsqueeze(-2).repeat_interleave(self.in_dim, dim=-2)


class DiffeqZeroTraceDeepSet(DiffeqNet):
    """``DiffeqZeroTraceDeepSet(dim, hidden_dims, k * dim, pooling='max')`` over sets (..., N, dim): elementwise MADE + exclusive
    pooling, [..., N, dim * k] dimension-major, and with ``return_log_det_jac`` (the default) zeros like x beside it.

    As in the reference, a `latent` passed here directly is concatenated onto x AHEAD of a MADE built for `in_dim` columns (so it
    only fits a net built for dim + latent columns); inside ``DiffeqExactTrace`` the exclusive net never receives one."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, pooling: str = 'max', return_log_det_jac: Optional[bool] = True,
                 **kwargs):
        super().__init__()
        self.elementwise = MADE(in_dim, hidden_dims, out_dim, return_per_dim=True)
        self.interaction = ZeroTraceEquivariantEncoder(in_dim, hidden_dims, out_dim // in_dim, pooling)
        self.return_log_det_jac = return_log_det_jac

    def forward(self, t, x, mask=None, latent=None, **kwargs):
        div = torch.zeros_like(x)
        if latent is not None:
            x = torch.cat([x, latent], -1)
        if mask is None:
            mask = torch.ones(*x.shape[:-1], 1).to(x)
        y = self.elementwise(x) + self.interaction(t, x, mask=mask)
        y = y * mask.unsqueeze(-1)
        y = y.reshape(*y.shape[:-2], -1)
        return (y, div) if self.return_log_det_jac else y


class DiffeqZeroTraceAttention(DiffeqNet):
    """``DiffeqZeroTraceAttention(dim, hidden_dims, k * dim, n_heads=1)`` over sets (..., N, dim), E = hidden_dims[-1]: q =
    MADE(dim, hidden_dims[:-1], E * dim) per dimension, k and v = MLP(dim, hidden_dims[:-1], E), proj = MLP(E, [], k); dim attentions
    with the diagonal masked against the same keys and values -> [..., N, dim * k] dimension-major, and with ``return_log_det_jac`` (the
    default) zeros like x beside it.  Ignores t and `latent`.  Runs on the HIP attention core with the (..., dim) leading dimensions
    flattened; differentiable.

    mask: None only.  (The reference's forward fails on a shape error for a mask of either shape its signature names; inside
    ``DiffeqExactTrace`` the exclusive net never receives one: DESIGN.md 4.14.)"""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, n_heads: int = 1, return_log_det_jac: Optional[bool] = True,
                 **kwargs):
        super().__init__()
        self.n_heads = n_heads
        self.return_log_det_jac = return_log_det_jac
        self.q = MADE(in_dim, hidden_dims[:-1], hidden_dims[-1] * in_dim, return_per_dim=True)
        self.k = MLP(in_dim, hidden_dims[:-1], hidden_dims[-1])
        self.v = MLP(in_dim, hidden_dims[:-1], hidden_dims[-1])
        self.proj = MLP(hidden_dims[-1], [], out_dim // in_dim)

    def forward(self, t, x, mask=None, latent=None, **kwargs):
        if mask is not None:
            raise NotImplementedError('DiffeqZeroTraceAttention: mask=None is the only supported call (the reference\'s forward raises a '
                                      'shape error for a mask; ContinuousTransform runs masked calls without handing it here)')
        D = x.shape[-1]
        query = self.q(x).transpose(-2, -3)                                       # (..., N, D, E) -> (..., D, N, E)
        key = self.k(x).unsqueeze(-3).expand(*x.shape[:-2], D, x.shape[-2], -1)   # the same keys and values for every dimension
        value = self.v(x).unsqueeze(-3).expand(*x.shape[:-2], D, x.shape[-2], -1)
        y = attention(query, key, value, self.n_heads, True, None).transpose(-2, -3)          # (..., N, D, E)
        y = self.proj(y)
        y = y.reshape(*y.shape[:-2], -1)
        return (y, torch.zeros_like(x)) if self.return_log_det_jac else y
