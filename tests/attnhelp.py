"""Helpers of the attention-CNF tests (fixture F20): cases rebuilt through the host classes, and the fixed grid of cnfhelp.solve64
restated over the closed form of the attention's per-element divergence (`net.self_attention_closed_form`: no autograd; the host
tests hold it against the autograd `divergence_exact_for_sets` and against the reference's own arrays).  `solve32` is the same
restatement evaluated in fp32: the fp32 sequence whose own error sets the bound (cnfhelp.bound) where fixture F20 holds no case -- the
module's composition path costs N * dim reverse passes WITH a graph per evaluation."""
import copy

import torch

import stribor_amd as st
from goldens import Golden

import cnfhelp as ch

_G = None
ACTS = ['Identity', 'Tanh', 'ReLU', 'Sigmoid', 'ELU', 'Softplus', 'LeakyReLU']


def golden():
    global _G
    if _G is None:
        _G = Golden('f20_attention_cnf')
    return _G


def case_names():
    return sorted(golden().meta['cases'])


def set_activation(module, act):
    """Replace the (Tanh) activation of the three embeddings by torch.nn.<act>() -- draws nothing."""
    att = module.odefunc.diffeq.net
    for m in (att.query, att.key, att.value):
        for i, layer in enumerate(list(m.net)):
            if not isinstance(layer, torch.nn.Linear):
                m.net[i] = getattr(torch.nn, act)()
        m.activation_name = act
    return module


def make(dim, hidden, n_heads=1, mask_diagonal=False, latent=0, T=1.0, solver='rk4', step=0.25, divergence='compute_set', set_data=True,
         act=None, biases=False):
    """An attention CNF in eval mode on the CPU (draws: the DiffeqSelfAttention's default init; `biases`: then every bias is drawn)."""
    net = st.net.DiffeqSelfAttention(dim + 1 + latent, hidden, dim, n_heads=n_heads, mask_diagonal=mask_diagonal)
    f = st.ContinuousTransform(dim, net=net, T=T, divergence=divergence, has_latent=latent > 0, solver=solver,
                               solver_options={'step_size': step}, set_data=set_data).eval()
    if act is not None:
        set_activation(f, act)
    if biases:
        with torch.no_grad():
            for n, p in f.named_parameters():
                if n.endswith('bias'):
                    p.normal_(0.0, 0.3)
    return f


def build_case(case):
    """-> (module in eval mode on the CPU, x, latent | None, meta): the fixture's construction and draws, in its order."""
    m = golden().meta['cases'][case]
    dim = m['shape'][-1]
    torch.manual_seed(m['seed'])
    net = st.net.DiffeqSelfAttention(dim + 1 + m['latent'], m['hidden'], dim, n_heads=m['n_heads'], mask_diagonal=m['mask_diagonal'])
    f = st.ContinuousTransform(dim, net=net, T=m['T'], divergence='compute_set', has_latent=m['latent'] > 0, solver=m['solver'],
                               solver_options=dict(m['options']), set_data=True).eval()
    x = torch.randn(*m['shape'])
    lat = torch.randn(*m['shape'][:-1], m['latent']) if m['latent'] else None
    assert torch.equal(x, golden().t(f'{case}/x'))
    return f, x, lat, m


def solve32(module, x, latent=None, reverse=False):
    return solve64(module, x, latent, reverse, dtype=torch.float32)


def solve64(module, x, latent=None, reverse=False, dtype=torch.float64):
    """The grid and tableau of cnfhelp.solve64 over the closed form, in `dtype` on the CPU -> (y, log-det [..., N, 1])."""
    solver = module.test_solver
    step = (module.test_solver_options or {}).get('step_size')
    t0, t1 = (module.T, 0.0) if reverse else (0.0, module.T)
    grid = ch.grid64(t0, t1, step)
    lat = None if latent is None else latent.detach().cpu().to(dtype)
    net = copy.deepcopy(module.odefunc.diffeq).cpu()
    want = module.odefunc.divergence != 'none'

    def aug(t, v):
        with torch.no_grad():
            dv, div = st.net.self_attention_closed_form(net, torch.tensor([t], dtype=dtype), v, lat, want_div=want, dtype=dtype)
        return dv, (div.sum(-1) if want else torch.zeros_like(v[..., 0]))

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
