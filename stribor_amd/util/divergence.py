"""Divergence of dy = f(y) by reverse mode (reference: stribor/util/divergence.py:5-22).  Torch ops; the composition path of
``ContinuousTransform`` uses them, its kernel path has the closed-form trace instead."""
import torch

__all__ = ['divergence_exact', 'divergence_approx', 'divergence_exact_for_sets']


def divergence_exact(output, input):
    """diag of d output / d input per feature, [..., dim]: one reverse pass per feature."""
    cols = [torch.autograd.grad(output[..., i].sum(), input, create_graph=True)[0][..., i] for i in range(input.shape[-1])]
    return torch.stack(cols, -1)


def divergence_exact_for_sets(output, input):
    """The same for set data [..., N, dim], where an element's output may depend on the other elements of its set."""
    rows = []
    for i in range(input.shape[-2]):
        cols = [torch.autograd.grad(output[..., i, j].sum(), input, create_graph=True)[0][..., i, j] for j in range(input.shape[-1])]
        rows.append(torch.stack(cols, -1))
    return torch.stack(rows, -2)


def divergence_approx(output, input, e, samples=1):
    """Hutchinson's estimator e^T J e, kept per feature: (J^T e) * e."""
    out = 0
    for _ in range(samples):
        out = out + torch.autograd.grad(output, input, e, create_graph=True)[0] * e / samples
    return out
