"""Differential-equation nets of the continuous normalizing flow (reference: stribor/net/diffeq.py:13-94).

Same constructors and ``state_dict`` keys (``net.net.0.weight``, ...); ``DiffeqMLP`` builds the product ``net.MLP``, so its
construction order and RNG draws are the MLP's.  The input columns are [t, x, latent] in this order (diffeq.py:44-47).
``ContinuousTransform`` does not call a ``DiffeqMLP`` on its kernel path at all: ``sx_cnf_flow`` consumes the weights directly.
``DiffeqDeepset`` is the same wrapper around ``net.EquivariantNet`` for sets of shape (..., N, dim) (keys
``net.layers.<i>.l1.weight``, ...); its kernel is ``sx_cnf_set_flow``.  ``DiffeqSelfAttention`` wraps ``net.SelfAttention`` (keys
``net.key.net.0.weight``, ..., ``net.proj.weight``; diffeq.py:97-113); its kernel is ``sx_cnf_attn_flow``.
"""
from abc import ABCMeta, abstractmethod
from typing import List

import torch
import torch.nn as nn

from .attention import SelfAttention
from .equivariant import EquivariantNet
from .mlp import MLP

__all__ = ['DiffeqNet', 'DiffeqConcat', 'DiffeqMLP', 'DiffeqDeepset', 'DiffeqSelfAttention']


class DiffeqNet(nn.Module, metaclass=ABCMeta):
    @abstractmethod
    def forward(self, t, x, latent=None, **kwargs):
        ...


class DiffeqConcat(DiffeqNet):
    """dx/dt = net([t, x, latent]) with the scalar time broadcast into a leading column (diffeq.py:25-48)."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, t, x, latent=None, **kwargs):
        cols = [torch.ones_like(x[..., :1]) * t, x]
        if latent is not None:
            cols.append(latent)
        inp = torch.cat(cols, -1)
        if type(self.net) is MLP and torch.is_grad_enabled():
            # the divergence differentiates this call, and training differentiates the divergence
            return self.net.forward_twice_differentiable(inp)
        if isinstance(self.net, SelfAttention) and type(self.net).forward is SelfAttention.forward and torch.is_grad_enabled():
            # the same for the attention: its HIP core and batch_linear are differentiable once
            return self.net.forward_twice_differentiable(inp, **kwargs)
        if isinstance(self.net, EquivariantNet) and type(self.net).forward is EquivariantNet.forward:
            # the same for the Deep Sets net, in every grad mode: the reference's op sequence, never the once-differentiable kernel
            return self.net.forward_twice_differentiable(inp, **kwargs)
        return self.net(inp, **kwargs)


class DiffeqMLP(DiffeqConcat):
    """``DiffeqMLP(dim + 1 (+ latent), hidden_dims, dim)`` (diffeq.py:51-75)."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, activation: str = 'Tanh',
                 final_activation: str = None, **kwargs):
        super().__init__(MLP(in_dim, hidden_dims, out_dim, activation, final_activation))


class DiffeqDeepset(DiffeqConcat):
    """``DiffeqDeepset(dim + 1 (+ latent), hidden_dims, dim)`` over sets (..., N, dim) (diffeq.py:78-94); ``mask`` reaches the
    equivariant layers through ``DiffeqConcat.forward``'s keyword arguments."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, activation: str = 'Tanh',
                 final_activation: str = None, **kwargs):
        super().__init__(EquivariantNet(in_dim, hidden_dims, out_dim, activation, final_activation))


class DiffeqSelfAttention(DiffeqConcat):
    """``DiffeqSelfAttention(dim + 1 (+ latent), hidden_dim, dim, n_heads, mask_diagonal)`` over sets (..., N, dim)
    (diffeq.py:97-113); ``mask`` reaches the attention through ``DiffeqConcat.forward``'s keyword arguments."""

    def __init__(self, in_dim: int, hidden_dim: List[int], out_dim: int, n_heads: int = 1, mask_diagonal: bool = False, **kwargs):
        super().__init__(SelfAttention(in_dim, hidden_dim, out_dim, n_heads, mask_diagonal))
