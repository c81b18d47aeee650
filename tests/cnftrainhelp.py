"""Helpers of the CNF training tests (test_cnf_train_host.py, test_gpu_cnf_train.py): modules, the fp64 truth of the Hutchinson solve
with its gradients (reverse mode twice, so it shares nothing with the kernels' closed form), and the per-tensor bound."""
import copy

import numpy as np
import torch

import stribor_amd as st

import cnfhelp as ch

ACTIVATIONS = ('Identity', 'Tanh', 'ReLU', 'Sigmoid', 'ELU', 'Softplus', 'LeakyReLU')
STAGES = {'euler': 1, 'midpoint': 2, 'rk4': 4}


def make(dim, hidden, latent=0, solver='rk4', step=0.25, T=0.7, activation='Tanh', seed=0, **kw):
    """A ContinuousTransform in training mode over a DiffeqMLP, every bias drawn (mlp.py zero-fills the last one)."""
    torch.manual_seed(seed)
    net = st.net.DiffeqMLP(dim + 1 + latent, hidden, dim, activation=activation, **kw.pop('net_kw', {}))
    with torch.no_grad():
        for l in net.net.net:
            if isinstance(l, torch.nn.Linear):
                l.bias.normal_(std=0.3)
    kw.setdefault('divergence', 'approximate')
    return st.ContinuousTransform(dim, net=net, T=T, has_latent=latent > 0, solver=solver, solver_options={'step_size': step}, **kw).train()


def linears(f):
    return [l for l in f.odefunc.diffeq.net.net if isinstance(l, torch.nn.Linear)]


def params(f):
    return [p for l in linears(f) for p in (l.weight, l.bias)]


def loss_of(y, ldj):
    """(-(unit normal log-density of y) - ldj).mean()"""
    d = y.shape[-1]
    return (0.5 * (y * y).sum(-1) + 0.5 * d * np.log(2 * np.pi) - ldj.reshape(y.shape[:-1])).mean()


def truth(f, x, e, lat=None, reverse=False, loss=loss_of):
    """The fp64 CPU restatement of the solve with the Hutchinson estimate for the noise `e` -> dict: y, ldj, loss, gx, glat, and the
    parameter gradients in `params(f)` order."""
    net = copy.deepcopy(f.odefunc.diffeq).double().cpu()
    ps = [p for l in net.net.net if isinstance(l, torch.nn.Linear) for p in (l.weight, l.bias)]
    for p in ps:
        p.requires_grad_(True)
    x64 = x.detach().cpu().double().requires_grad_(True)
    e64 = e.detach().cpu().double()
    lat64 = None if lat is None else lat.detach().cpu().double().requires_grad_(True)
    t0, t1 = (f.T, 0.0) if reverse else (0.0, f.T)
    grid = ch.grid64(t0, t1, (f.solver_options or {}).get('step_size'))

    def aug(t, v):
        dv = net(torch.tensor([t], dtype=torch.float64), v, latent=lat64)
        q = (torch.autograd.grad(dv, v, e64, create_graph=True)[0] * e64).sum(-1)
        return dv, q

    y, l = x64, torch.zeros(x64.shape[:-1], dtype=torch.float64)
    for ta, tb in zip(grid[:-1], grid[1:]):
        dt = tb - ta
        k1, q1 = aug(ta, y)
        if f.solver == 'euler':
            y, l = y + dt * k1, l + dt * q1
        elif f.solver == 'midpoint':
            k2, q2 = aug(ta + dt / 2, y + dt / 2 * k1)
            y, l = y + dt * k2, l + dt * q2
        else:
            k2, q2 = aug(ta + dt / 3, y + dt * k1 / 3)
            k3, q3 = aug(ta + 2 * dt / 3, y + dt * (k2 - k1 / 3))
            k4, q4 = aug(tb, y + dt * (k1 - k2 + k3))
            y, l = y + dt * (k1 + 3 * (k2 + k3) + k4) / 8, l + dt * (q1 + 3 * (q2 + q3) + q4) / 8
    L = loss(y, l)
    wrt = [x64] + ([] if lat64 is None else [lat64]) + ps
    g = torch.autograd.grad(L, wrt, allow_unused=True)
    g = [torch.zeros_like(w) if a is None else a for a, w in zip(g, wrt)]
    n_in = 1 if lat64 is None else 2
    return {'y': y.detach(), 'ldj': l.detach().unsqueeze(-1), 'loss': L.detach(), 'gx': g[0], 'glat': None if lat64 is None else g[1],
            'params': g[n_in:]}


def run(f, x, lat=None, reverse=False, mask=None, seed=11, loss=loss_of):
    """One training call of `f` on the GPU and its backward -> dict like `truth` (fp32, on the device) plus e and the path taken.
    `mask` of ones forces the composition path (DiffeqMLP ignores it)."""
    for p in f.parameters():
        p.grad = None
    x = x.detach().clone().requires_grad_(True)
    lat = None if lat is None else lat.detach().clone().requires_grad_(True)
    torch.manual_seed(seed)
    y, ldj = f.forward_and_log_det_jacobian(x, latent=lat, mask=mask, reverse=reverse)
    path, evals = f._last_path, f._num_evals()
    e = f.odefunc._e
    loss(y, ldj).backward()
    return {'y': y.detach(), 'ldj': ldj.detach(), 'gx': x.grad, 'glat': None if lat is None else lat.grad,
            'params': [p.grad for p in params(f)], 'e': e, 'path': path, 'evals': evals}


def check(tag, got, ref, want, n_evals):
    """Every tensor of `got` within cnfhelp.bound of `want` (8 x the composition path's own fp32 error, floor 1e-6 max(1, max |want|);
    parameter gradients: floor 8 K 2^-23 max(1, max |want|), K = evaluations) -> the worst error / bound ratio."""
    worst, fails = 0.0, []
    names = ['y', 'ldj', 'gx'] + (['glat'] if want['glat'] is not None else [])
    items = [(k, got[k], ref[k], want[k], None) for k in names]
    items += [(f'param{i}', a, b, c, n_evals) for i, (a, b, c) in enumerate(zip(got['params'], ref['params'], want['params']))]
    for name, a, r, t, k in items:
        tol, e_ref = ch.bound(r.detach().cpu(), t)
        if k is not None:
            tol = max(8 * e_ref, 8 * k * 2.0 ** -23 * max(1.0, t.abs().max().item() if t.numel() else 0.0))
        err = (a.detach().cpu().double() - t).abs().max().item() if t.numel() else 0.0
        worst = max(worst, err / tol)
        if not err <= tol:
            fails.append((name, err, e_ref, tol))
    print(f'{tag}: worst error / bound {worst:.3f}')
    assert not fails, (tag, fails)
    return worst
