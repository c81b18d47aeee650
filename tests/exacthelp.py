"""Helpers of the exact-trace CNF tests: fixture F17 cases rebuilt through the host classes, and an fp64 restatement of
DiffeqExactTraceMLP as the UN-DETACHED composition (plain torch ops; its Jacobian diagonal comes from reverse-mode autograd, so it
shares nothing with FuncAndDiagJac's cut or with the kernel's forward-mode tangent)."""
import torch

import stribor_amd as st
from goldens import Golden

_G = None


def golden():
    global _G
    if _G is None:
        _G = Golden('f17_exact_trace')
    return _G


def case_names():
    return sorted(golden().meta['cases'])


def construct(m, seed=None):
    """The fixture's construction under its seed (weights and biases draw for draw; the masks are the constructor's own draw)."""
    dim = m['shape'][-1]
    torch.manual_seed(m['seed'] if seed is None else seed)
    net = st.net.DiffeqExactTraceMLP(dim, m['hidden'], dim, m['d_h'], latent_dim=m['latent'])
    return st.ContinuousTransform(dim, net=net, T=m['T'], divergence='exact', has_latent=m['latent'] > 0, solver=m['solver'],
                                  solver_options=dict(m['options'])).eval()


def build_case(case):
    """-> (module in eval mode on the CPU with the fixture's state, x, latent | None, meta)."""
    g = golden()
    m = g.meta['cases'][case]
    f = construct(m)
    f.load_state_dict(g.state(case), strict=True)
    return f, g.t(f'{case}/x'), (g.t(f'{case}/latent') if g.has(f'{case}/latent') else None), m


def set_activation(net, act):
    """One of torch's activations by hand on the three nets of a DiffeqExactTraceMLP (the reference's constructors offer no argument
    for it): the two MADEs and the dimwise MLP, as exactsethelp.set_activation does for the set net."""
    made1, made2, dw = net.exclusive_net.net1, net.exclusive_net.net2, net.dimwise_net.net
    made1.activation = made2.activation = dw.activation_name = act
    for seq in (made1.net, made2.net, dw.net):
        for i in range(1, len(seq), 2):
            seq[i] = getattr(torch.nn, act)()
    return net


def net64(net, latent=None):
    """fp64 restatement of a DiffeqExactTraceMLP-shaped module (MADE + MADE, then the dimwise MLP over [t, x_i, h_i, latent]) as one
    differentiable function f(t, x) -> [..., D] on the CPU; `params`: substitute tensors keyed like net.named_parameters()."""
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    return lambda t, v: apply64(net, sd, t, v, None if latent is None else latent.detach().cpu().double())


def apply64(net, sd, t, v, latent=None):
    def stack(prefix, module, a, masked):
        for i, layer in enumerate(module):
            if isinstance(layer, torch.nn.Linear):
                W = sd[f'{prefix}.{i}.weight']
                if masked:
                    W = sd[f'{prefix}.{i}.mask'] * W
                a = torch.nn.functional.linear(a, W, sd.get(f'{prefix}.{i}.bias'))
            else:
                a = layer(a)
        return a
    D = v.shape[-1]
    raw = (stack('exclusive_net.net1.net', net.exclusive_net.net1.net, v, True)
           + stack('exclusive_net.net2.net', net.exclusive_net.net2.net, v, True))
    h = raw.reshape(*v.shape[:-1], -1, D).transpose(-1, -2)                     # [..., D, d_h]
    cols = [torch.ones_like(v).unsqueeze(-1) * t, v.unsqueeze(-1), h]
    if latent is not None:
        cols.append(latent.unsqueeze(-2).expand(*v.shape, latent.shape[-1]))
    return stack('dimwise_net.net.net', net.dimwise_net.net.net, torch.cat(cols, -1), False).squeeze(-1)


def diag64(f, t, x):
    """(f(t, x), its Jacobian diagonal) by one reverse pass per dimension."""
    with torch.enable_grad():
        v = x.detach().cpu().double().requires_grad_(True)
        dv = f(t, v)
        diag = torch.stack([torch.autograd.grad(dv[..., i].sum(), v, retain_graph=True)[0][..., i] for i in range(v.shape[-1])], -1)
    return dv.detach(), diag.detach()
