"""What the one-launch kernels ask of a module, stated once for every planner (``flows.cnf``, ``flows.iresnet``,
``net.diffeq_exact_trace``): the activation, tensor and layer-stack conditions, the tile count, and the activations themselves as
torch ops with the derivatives the kernels take."""
import torch
import torch.nn as nn

from .. import _hip

_DEFAULTS = {nn.LeakyReLU: lambda m: m.negative_slope == 0.01, nn.ELU: lambda m: m.alpha == 1.0,
             nn.Softplus: lambda m: m.beta == 1 and m.threshold == 20}
_zero = lambda h, d: torch.zeros_like(h)

# name -> (act(a), act'(h), act''(h, act'(h))): both derivatives from the activation's OUTPUT h = act(a), as the kernels take them
ACTS = {'Identity': (lambda a: a, torch.ones_like, _zero),
        'Tanh': (torch.tanh, lambda h: 1 - h * h, lambda h, d: -2 * h * d),
        'ReLU': (torch.relu, lambda h: (h > 0).to(h.dtype), _zero),
        'Sigmoid': (torch.sigmoid, lambda h: h * (1 - h), lambda h, d: d * (1 - 2 * h)),
        'ELU': (nn.functional.elu, lambda h: torch.where(h > 0, torch.ones_like(h), h + 1),
                lambda h, d: torch.where(h > 0, torch.zeros_like(h), h + 1)),
        'Softplus': (nn.functional.softplus, lambda h: 1 - torch.exp(-h), lambda h, d: d * (1 - d)),
        'LeakyReLU': (nn.functional.leaky_relu, lambda h: torch.where(h > 0, torch.ones_like(h), torch.full_like(h, 0.01)), _zero)}


def kernel_activation(name, modules=()) -> bool:
    """Is `name` one of the seven activations with an in-kernel derivative, and is every module of `modules` the plain ``torch.nn``
    class of that name with torch's DEFAULT parameters (the only ones the kernels evaluate)?"""
    if _hip.ACT_CODES.get(name, 99) > 6:
        return False
    return all(type(m) is getattr(nn, name) and _DEFAULTS.get(type(m), lambda m: True)(m) is True for m in modules)


def kernel_tensors(tensors, device) -> bool:
    """Can a kernel read every tensor in place: present, fp32, contiguous and on `device`?"""
    return all(t is not None and t.dtype == torch.float32 and t.is_contiguous() and t.device == device for t in tensors)


def linear_stack(seq, final_activation: bool = False):
    """The Linear layers of an ``MLP``-style ``nn.Sequential`` when it is exactly ``Linear (act Linear)* [final act]``, else None."""
    layers = list(seq)
    if final_activation:
        if not layers or isinstance(layers[-1], nn.Linear):
            return None
        layers.pop()
    if len(layers) % 2 != 1 or any(isinstance(m, nn.Linear) != (i % 2 == 0) for i, m in enumerate(layers)):
        return None
    return layers[0::2]


def tiles(n: int) -> int:
    """Tiles of 32 that hold `n` columns (1, 2 or 4): ``cnf_tiles`` of csrc/sx_cnf_common.h."""
    return 1 if n <= 32 else 2 if n <= 64 else 4
