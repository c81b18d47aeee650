"""Permutation-equivariant layers over sets of shape (..., N, dim) (reference: stribor/net/equivariant.py:6-93).

Same constructors, ``state_dict`` keys (``layers.<i>.l1.weight``, ``layers.<i>.l2.weight``, ...) and RNG draws: per layer ``l1`` then
``l2``, both default-initialised ``nn.Linear``.  Plain differentiable torch modules for any device: the composition path of
``ContinuousTransform``, training and the CPU restatements run them.  On its kernel path ``ContinuousTransform`` does not call them:
``sx_cnf_set_flow`` consumes the weights directly.
"""
from typing import List

import torch.nn as nn

__all__ = ['EquivariantLayer', 'EquivariantNet']


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


class EquivariantNet(nn.Module):
    """``EquivariantNet(in_dim, hidden_dims, out_dim, activation='Tanh', final_activation=None)``: ``net.MLP``'s arguments with
    ``EquivariantLayer`` in place of ``nn.Linear`` (equivariant.py:45-93).

    >>> net = stribor_amd.net.EquivariantNet(2, [64, 64], 4)
    """

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, activation: str = 'Tanh', final_activation: str = None,
                 **kwargs):
        super().__init__()
        self.activation = getattr(nn, activation)()
        self.final_activation = getattr(nn, final_activation)() if final_activation else nn.Identity()
        dims = [in_dim] + list(hidden_dims) + [out_dim]
        self.layers = nn.ModuleList([EquivariantLayer(a, b) for a, b in zip(dims[:-1], dims[1:])])

    def forward(self, x, mask=None, **kwargs):
        for layer in self.layers[:-1]:
            x = self.activation(layer(x, mask=mask))
        return self.final_activation(self.layers[-1](x, mask=mask))
