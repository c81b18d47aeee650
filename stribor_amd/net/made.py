"""Masked autoregressive MLP (reference: stribor/net/made.py; Germain et al., "MADE", arXiv:1502.03509).

Same constructor, same ``state_dict`` keys (``net.{0,2,...}.{weight,bias,mask}``): the masks are float buffers of the weight's shape
``[out, in]``, drawn from an UNSEEDED numpy generator, so they travel with a checkpoint and cannot be rebuilt from a torch seed.
``forward`` is plain torch (``F.linear(x, mask * weight, bias)``): differentiable to any order on any device.  Inside an exact-trace
CNF the kernel path does not call a MADE at all: ``sx_cnf_exact_flow`` consumes ``mask * weight`` (net/diffeq_exact_trace.py).
"""
from typing import List

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..fused import StructureTracked

__all__ = ['MADE', 'MaskedLinear']


class MaskedLinear(StructureTracked, nn.Linear):
    """nn.Linear (same initialisation, same RNG draws) whose weight is multiplied by a fixed 0 / 1 mask.  A re-assigned weight, bias
    or mask invalidates the cached kernel images that staged the old tensors (StructureTracked, like net.mlp._Linear)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True):
        super().__init__(in_features, out_features, bias)
        self.register_buffer('mask', torch.ones(out_features, in_features))

    def set_mask(self, mask):
        """mask: numpy [in, out] (the orientation the degrees are compared in); copied in place, so cache guards see a new version."""
        with torch.no_grad():
            self.mask.copy_(torch.from_numpy(np.ascontiguousarray(mask.T).astype(np.float32)))

    def masked_weight(self):
        return self.mask * self.weight

    def forward(self, input):
        return F.linear(input, self.mask * self.weight, self.bias)


class MADE(StructureTracked, nn.Module):
    """out_dim = k * in_dim outputs; output column j * in_dim + i belongs to input dimension i and depends only on the inputs that
    come before i in the ordering.

    Degrees: the inputs carry their rank in the ordering (natural 0 .. in_dim - 1, reversed, or a random permutation); a hidden unit
    draws a degree in [min of the previous layer's degrees, max(in_dim - 1, 1)); a connection into a hidden unit needs
    degree_in <= degree_out, a connection into an output needs degree_hidden < rank of the output's dimension, and that last mask
    is repeated k times.  ``update_masks`` redraws (only when ``num_masks`` > 1: a single mask is drawn once).

    return_per_dim: [..., in_dim, k] instead of [..., in_dim * k] (dimension-major either way)."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, activation: str = 'Tanh', final_activation: str = None,
                 num_masks: int = 1, natural_ordering: bool = False, reverse_ordering: bool = False, return_per_dim: bool = False,
                 **kwargs):
        super().__init__()
        if out_dim % in_dim != 0:
            raise AssertionError('out_dim must be integer multiple of in_dim')
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.hidden_dims = hidden_dims
        self.activation = activation
        self.final_activation = final_activation
        self.return_per_dim = return_per_dim
        self.natural_ordering = natural_ordering
        self.reverse_ordering = reverse_ordering
        self.num_masks = num_masks
        widths = [in_dim] + list(hidden_dims) + [out_dim]
        layers = []
        for i in range(len(widths) - 1):
            if i:
                layers.append(getattr(nn, activation)())
            layers.append(MaskedLinear(widths[i], widths[i + 1]))
        if final_activation is not None:
            layers.append(getattr(nn, final_activation)())
        self.net = nn.Sequential(*layers)
        self.m = {}
        self.update_masks()

    def masked_linears(self):
        return [l for l in self.net if isinstance(l, MaskedLinear)]

    def update_masks(self):
        if self.m and self.num_masks == 1:
            return
        rng = np.random.RandomState()
        n_hidden = len(self.hidden_dims)
        if self.natural_ordering:
            order = np.arange(self.in_dim)
            self.m[-1] = order[::-1] if self.reverse_ordering else order
        else:
            self.m[-1] = rng.permutation(self.in_dim)
        top = max(self.in_dim - 1, 1)
        for l in range(n_hidden):
            self.m[l] = rng.randint(self.m[l - 1].min(), top, size=self.hidden_dims[l])
        masks = [self.m[l - 1][:, None] <= self.m[l][None, :] for l in range(n_hidden)]
        last = self.m[n_hidden - 1][:, None] < self.m[-1][None, :]
        masks.append(np.tile(last, (1, self.out_dim // self.in_dim)))
        for layer, mask in zip(self.masked_linears(), masks):
            layer.set_mask(mask)

    def forward(self, x, **kwargs):
        lead = x.shape[:-1]
        y = self.net(x.reshape(-1, x.shape[-1]))
        y = y.reshape(*lead, -1, self.in_dim).transpose(-1, -2)          # column j * in_dim + i -> [i, j]
        return y if self.return_per_dim else y.reshape(*lead, -1)
