"""Softmax that maps an all -inf row to zeros (reference: stribor/util/safe_softmax.py:3-14).

Not on the hot path: the attention nets run their softmax inside the HIP attention core, which gives the same zeros.
"""
import torch


def safe_softmax(x: torch.Tensor, dim: int = -1) -> torch.Tensor:
    """torch.softmax along `dim`, with the NaNs of an all -inf row replaced by 0 (such a row then sums to 0, not 1)."""
    return torch.nan_to_num(torch.softmax(x, dim))
