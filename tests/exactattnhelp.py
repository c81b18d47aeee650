"""Helpers of the exact-trace attention set-CNF tests (fixture F22): cases rebuilt through the host classes, and the fixed grid restated
in fp32 / fp64 over ``net.diffeq_exact_trace.closed_form_attn`` (which test_exact_attn_host.py holds to autograd's Jacobian in fp64).
`solve32` is the fp32 sequence whose own error sets the bound (cnfhelp.bound) where F22 holds no case."""
import torch

import stribor_amd as st
from stribor_amd.net import diffeq_exact_trace as xt
from goldens import Golden

import cnfhelp as ch

_G = None


def golden():
    global _G
    if _G is None:
        _G = Golden('f22_exact_attn')
    return _G


def case_names():
    return sorted(golden().meta['cases'])


def make(dim, hidden, d_h, latent=0, heads=1, T=1.0, solver='rk4', step=0.25, seed=0, net=None, biases=True, **kw):
    """An exact-trace attention set CNF in eval mode on the CPU.  `biases`: every bias drawn non-zero (mlp.py zero-fills the MLPs' last
    ones)."""
    torch.manual_seed(seed)
    net = net or xt.DiffeqExactTraceAttention(dim, hidden, dim, d_h, latent_dim=latent, n_heads=heads)
    if biases:
        with torch.no_grad():
            for k, p in net.named_parameters():
                if k.endswith('bias'):
                    p.normal_(0, 0.3)
    return st.ContinuousTransform(dim, net=net, T=T, divergence='exact', has_latent=latent > 0, solver=solver,
                                  solver_options={'step_size': step}, **kw).eval()


def build_case(case):
    """-> (module in eval mode on the CPU with the fixture's state, x, latent | None, meta): weights and biases are the construction's
    draws under the case's seed (held to the fixture's hashes), the q MADE's masks come from the fixture."""
    g = golden()
    m = g.meta['cases'][case]
    dim = m['shape'][-1]
    torch.manual_seed(m['seed'])
    net = xt.DiffeqExactTraceAttention(dim, m['hidden'], dim, m['d_h'], latent_dim=m['latent'], n_heads=m['heads'])
    f = st.ContinuousTransform(dim, net=net, T=m['T'], divergence='exact', has_latent=m['latent'] > 0, solver=m['solver'],
                               solver_options=dict(m['options'])).eval()
    state = f.state_dict()
    for k, want in m['state_sha256'].items():
        assert ch.sha(state[k]) == want, f'{case}: state tensor {k} differs from the reference\'s'
    masks = g.state(case)
    assert sorted(masks) == sorted(k for k in state if k.endswith('mask'))
    f.load_state_dict(masks, strict=False)
    return f, g.t(f'{case}/x'), (g.t(f'{case}/latent') if g.has(f'{case}/latent') else None), m


def solve32(module, x, latent=None, reverse=False):
    return solve64(module, x, latent, reverse, dtype=torch.float32)


def solve64(module, x, latent=None, reverse=False, dtype=torch.float64):
    """The grid and tableau of cnfhelp.solve64 over closed_form_attn in `dtype`, on the CPU -> (y, log-det [..., N, 1])."""
    solver = module.test_solver
    step = (module.test_solver_options or {}).get('step_size')
    t0, t1 = (module.T, 0.0) if reverse else (0.0, module.T)
    grid = ch.grid64(t0, t1, step)
    net = module.odefunc.diffeq
    lat = None if latent is None else latent.detach().cpu().to(dtype)

    def aug(t, v):
        f, jac = xt.closed_form_attn(net, t, v, lat, dtype=dtype)
        return f, jac.sum(-1)

    y, l = x.detach().cpu().to(dtype), torch.zeros(x.shape[:-1], dtype=dtype)
    for ta, tb in zip(grid[:-1], grid[1:]):
        dt = tb - ta
        k1, q1 = aug(ta, y)
        if solver == 'euler':
            y, l = y + dt * k1, l + dt * q1
        elif solver == 'midpoint':
            k2, q2 = aug(ta + dt / 2, y + dt / 2 * k1)
            y, l = y + dt * k2, l + dt * q2
        else:
            k2, q2 = aug(ta + dt / 3, y + dt * k1 / 3)
            k3, q3 = aug(ta + 2 * dt / 3, y + dt * (k2 - k1 / 3))
            k4, q4 = aug(tb, y + dt * (k1 - k2 + k3))
            y, l = y + dt * (k1 + 3 * (k2 + k3) + k4) / 8, l + dt * (q1 + 3 * (q2 + q3) + q4) / 8
    return y, l.unsqueeze(-1)


def set_activation(net, act, instance=None):
    """One of torch's activations by hand on the nets of a DiffeqExactTraceAttention (the reference's constructors offer no argument
    for it).  `instance`: a factory for the modules (non-default parameters)."""
    import torch.nn as nn
    ex, dw = net.exclusive_net, net.dimwise_net.net
    ex.q.activation = ex.k.activation_name = ex.v.activation_name = ex.proj.activation_name = dw.activation_name = act
    for seq in (ex.q.net, ex.k.net, ex.v.net, dw.net):
        for i in range(1, len(seq), 2):
            seq[i] = instance() if instance else getattr(nn, act)()
    return net
