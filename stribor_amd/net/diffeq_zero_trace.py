"""Zero-trace differential-equation net (reference: stribor/net/diffeq_zero_trace.py:14-56): for ``divergence='exact'``.

``DiffeqZeroTraceMLP`` is the sum of two MADEs in the natural ordering, one of them reversed: output i of the first depends on the
inputs before i, of the second on the inputs after i, so together on every input but x_i -- the Jacobian is hollow and its trace 0.
Same constructor and ``state_dict`` keys (``net1.net.0.{weight,bias,mask}``, ``net2...``); ``net1`` is built (and draws) first.
"""
from typing import List, Optional

import torch

from .diffeq import DiffeqNet
from .made import MADE

__all__ = ['DiffeqZeroTraceMLP']


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
