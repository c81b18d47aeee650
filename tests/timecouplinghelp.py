"""Helpers of the ContinuousAffineCoupling training tests (test_time_coupling_train_host.py, test_gpu_time_coupling_train.py): layers
built through the product classes, their oracle specs over fp64 leaves, and the fp64 truth of a call's gradients by autograd of
oracle.continuous_affine_coupling (which shares nothing with the kernel's closed form)."""
import torch

import stribor_amd as st
from oracle import stribor_oracle as orc

TIME = {'identity': st.net.TimeIdentity, 'linear': st.net.TimeLinear, 'tanh': st.net.TimeTanh, 'log': st.net.TimeLog}
ACTIVATIONS = ('Identity', 'Tanh', 'ReLU', 'Sigmoid', 'ELU', 'Softplus', 'LeakyReLU')
# (method, reverse, sigma, the loss uses the log-det)
MODES = {'forward': (False, 1.0, False), 'inverse': (True, 1.0, False), 'forward_and_log_det_jacobian': (False, 1.0, True),
         'inverse_and_log_det_jacobian': (True, -1.0, True)}


def make_layer(D, H, L, kind='tanh', half=None, concat=True, act='Tanh', mask='ordered_left_half', seed=0, hidden=None):
    """A ContinuousAffineCoupling on the CPU with every parameter drawn (the last Linear's bias too: mlp.py:53 zeroes it)."""
    torch.manual_seed(seed)
    net = st.net.MLP(D + L + int(concat), list(hidden or [H]), 2 * D, activation=act)
    tn = TIME[kind](2 * (D if half is None else half)) if kind in TIME else kind
    f = st.ContinuousAffineCoupling(net, tn, mask, concatenate_time=concat)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0.0, 0.3)
    return f


def layer_spec(f, leaves, prefix=''):
    """The oracle's spec of `f` over `leaves` (name -> fp64 tensor, the layer's own parameter names behind `prefix`)."""
    lins = [(n, m) for n, m in f.latent_net.net.named_children() if isinstance(m, torch.nn.Linear)]
    tn = f.time_net
    kind = {v: k for k, v in TIME.items()}.get(type(tn), 'fourier')
    D = lins[-1][1].weight.shape[0] // 2
    return {'mask': f._oracle_mask, 'concatenate_time': bool(f.concatenate_time), 'time_kind': kind, 'time_out': 2 * D,
            'time_scale': leaves.get(prefix + 'time_net.scale'), 'time_weight': leaves.get(prefix + 'time_net.weight'),
            'time_shift': leaves.get(prefix + 'time_net.shift'),
            'net': {'weights': [leaves[f'{prefix}latent_net.net.{n}.weight'] for n, _ in lins],
                    'biases': [leaves[f'{prefix}latent_net.net.{n}.bias'] for n, _ in lins], 'activation': f.latent_net.activation_name}}


class oracle_masks:
    """Pins each layer's mask to the vector it holds now (a layer keeps its 'random_half' draw only until its caches are dropped) and
    makes the oracle's mask_vector hand back those vectors for the names the layers are given as `_oracle_mask` (the oracle does not
    draw 'random_half')."""

    def __init__(self, monkeypatch, layers, D):
        self.table = {}
        for i, f in enumerate(layers):
            f._oracle_mask = f'layer{i}'
            drawn = f.mask_func(D).clone()
            f.mask_func = lambda dim, drawn=drawn: drawn.clone()
            self.table[f._oracle_mask] = drawn
        monkeypatch.setattr(orc, 'mask_vector', lambda name, dim: self.table[name])


def leaves_of(module):
    return {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in module.named_parameters()}


def inputs(n, D, L, seed, t_scale=2.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g)
    t = torch.rand(n, 1, generator=g) * t_scale
    lat = torch.randn(n, L, generator=g) if L else None
    wy = torch.randn(n, D, generator=g)
    wl = torch.randn(n, 1, generator=g)
    return x, t, lat, wy, wl


def loss_of(y, ldj, wy, wl, uses_ldj):
    loss = (y * wy).sum()
    return loss + (ldj * wl).sum() if uses_ldj else loss


def truth(f, mode, x, t, lat, wy, wl, weight=None):
    """fp64 autograd of the oracle -> {'x', 't', 'latent', parameter name: gradient}.  `weight` [n, 1]: how often each row counts."""
    reverse, sigma, uses = MODES[mode]
    leaves = leaves_of(f)
    spec = layer_spec(f, leaves)
    xs = [v if v is None else v.double().clone().requires_grad_(True) for v in (x, t, lat)]
    y, ldj = orc.continuous_affine_coupling(spec, xs[0], xs[1], xs[2], reverse)
    w = 1.0 if weight is None else weight.double()
    loss_of(y * w, sigma * ldj * w, wy.double(), wl.double(), uses).backward()
    out = {'x': xs[0].grad, 't': xs[1].grad, 'latent': None if lat is None else xs[2].grad}
    out.update({k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()})
    return out


def run(f, mode, x, t, lat, wy, wl, composed=False, needs=(True, True, True)):
    """One graph-building call of `f` (on its own device) and its backward -> the gradients, named as `truth` names them."""
    reverse, sigma, uses = MODES[mode]
    dev = next(f.parameters()).device
    xs = [None if v is None else v.to(dev).clone().requires_grad_(r) for v, r in zip((x, t, lat), needs)]
    f.zero_grad(set_to_none=True)
    if composed:
        y, ldj = f._run_composed(xs[0], xs[1], xs[2], reverse, uses, sigma)
    else:
        y = getattr(f, mode)(xs[0], xs[1], latent=xs[2])
        y, ldj = y if uses else (y, None)
    loss_of(y, ldj, wy.to(dev), wl.to(dev), uses).backward()
    out = {k: (None if v is None else v.grad) for k, v in zip(('x', 't', 'latent'), xs)}
    out.update({k: v.grad for k, v in f.named_parameters()})
    return out, y.detach(), (None if ldj is None else ldj.detach())
