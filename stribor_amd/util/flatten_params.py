"""All parameters of some modules as one flat tensor (reference: stribor/util/flatten_params.py): the handle through which
``net.FuncAndDiagJac`` hands parameter gradients back to autograd."""
import torch

__all__ = ['flatten_params']


def flatten_params(*nets):
    flat = [p.contiguous().view(-1) for net in nets for p in net.parameters()]
    return torch.cat(flat) if flat else torch.tensor([])
