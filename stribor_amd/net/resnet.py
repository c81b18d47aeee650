"""Residual networks over this package's ``net.MLP`` (reference: stribor/net/resnet.py): ``ResNetBlock`` is ``x + g(x)`` with ``g`` an
MLP from ``dim`` to ``dim``, ``ResNet`` a chain of such blocks.  ``state_dict`` keys are ``net.{i}.net.net.{2j}.{weight,bias}``.  As a
``Coupling`` conditioner a ``ResNet`` takes the any-``nn.Module`` tier: each block's MLP runs as its own program, the sums are torch ops.
"""
from typing import List, Optional

import torch.nn as nn

from .mlp import MLP

__all__ = ['ResNet', 'ResNetBlock']


class ResNetBlock(nn.Module):
    def __init__(self, dim: int, hidden_dims: List[int], activation: str = 'ReLU', final_activation: Optional[str] = None, **kwargs):
        super().__init__()
        self.net = MLP(dim, hidden_dims, dim, activation, final_activation)

    def forward(self, x):
        return x + self.net(x)


class ResNet(nn.Module):
    def __init__(self, dim: int, hidden_dims: List[int], num_layers: int, activation: str = 'ReLU',
                 final_activation: Optional[str] = None, **kwargs):
        super().__init__()
        self.net = nn.Sequential(*[ResNetBlock(dim, hidden_dims, activation, final_activation) for _ in range(num_layers)])

    def forward(self, x, **kwargs):
        return self.net(x)
