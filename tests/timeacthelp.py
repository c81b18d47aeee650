"""Helpers of the ContinuousTanh / ContinuousActivation tests: restatements of the two formulas (the reference's literal sequence,
activations.py:149-150 and :176-192, in the dtype of their inputs -- fp32 for the reference's own error, fp64 for the truth), their
gradients by fp64 autograd, the tolerance, and a mixed-flow restatement over the oracle's continuous_affine_coupling."""
import torch

import cnfhelp
import stribor_amd as st
from goldens import Golden
from oracle import stribor_oracle as orc
from stribor_amd.util import flowdesc as fd

_G = None
ACTS = {'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu}


def golden():
    global _G
    if _G is None:
        _G = Golden('f24_time_activations')
    return _G


def tanh_flow(x, t, log_time=False, reverse=False):
    """activations.py:176-180, literally."""
    if log_time:
        t = torch.log1p(t)
    if reverse:
        t = -t
    return torch.asinh(t.exp() * torch.sinh(x))


def tanh_flow_ldiag(x, t, log_time=False, reverse=False):
    """activations.py:188-192, literally (reverse: of the inverse map, i.e. at -t)."""
    if log_time:
        t = torch.log1p(t)
    if reverse:
        t = -t
    t = t.exp()
    return (t * torch.cosh(x) / torch.sqrt(torch.square(t * torch.sinh(x)) + 1)).log()


def mix(name, x, t, temperature):
    """activations.py:149-150, literally."""
    w = torch.tanh(temperature * t)
    return x * (1 - w) + ACTS[name](x) * w


def bound(ref32, truth64):
    """cnfhelp.bound with the reference's error taken over the entries where its fp32 result is finite; the floor over every entry."""
    fin = torch.isfinite(ref32)
    tol, e_ref = cnfhelp.bound(ref32[fin], truth64[fin])
    floor = 1e-6 * max(1.0, truth64.abs().max().item() if truth64.numel() else 0.0)
    return max(tol, floor), e_ref


def check(got, ref32, truth64, what):
    """got (device tensor) against the fp64 truth under `bound`; prints the figures before it asserts."""
    tol, e_ref = bound(ref32, truth64)
    got = got.detach().cpu().double()
    assert got.shape == truth64.shape, (what, got.shape, truth64.shape)
    assert torch.isfinite(got).all(), f'{what}: non-finite result'
    err = (got - truth64).abs().max().item() if truth64.numel() else 0.0
    print(f'{what}: err {err:.3e} tol {tol:.3e} (reference fp32 err {e_ref:.3e})')
    assert err <= tol, f'{what}: err {err:.3e} > tol {tol:.3e} (reference fp32 err {e_ref:.3e})'


def rows_like(t, x):
    return t.expand(*x.shape[:-1], 1)


def flow_grads(x, t, gy, gld, log_time, reverse, dtype):
    """(gx, gt) of sum(y * gy) + sum(ldiag * gld) for the tanh-flow restatement in `dtype`, by autograd; t has x's leading shape + (1,)."""
    x = x.detach().to(dtype).requires_grad_(True)
    t = t.detach().to(dtype).requires_grad_(True)
    loss = (tanh_flow(x, t, log_time, reverse) * gy.to(dtype)).sum() + (tanh_flow_ldiag(x, t, log_time, reverse) * gld.to(dtype)).sum()
    gx, gt = torch.autograd.grad(loss, (x, t))
    return gx, gt


def mix_grads(name, x, t, temperature, gy, dtype):
    """(gx, gt, gtemperature) of sum(y * gy) for the mix restatement in `dtype`."""
    x = x.detach().to(dtype).requires_grad_(True)
    t = t.detach().to(dtype).requires_grad_(True)
    temp = torch.tensor(temperature, dtype=dtype, requires_grad=True)
    loss = (mix(name, x, t, temp) * gy.to(dtype)).sum()
    return torch.autograd.grad(loss, (x, t, temp))


# ---- mixed flows: couplings of fixture F11's construction with the time-dependent activations between them ---------------------------
def coupling_desc(dim, mask, latent_dim=0, hidden=13):
    return {'kind': 'continuous_affine_coupling', 'dim': dim, 'hidden': [hidden], 'mask': mask, 'latent_dim': latent_dim,
            'time_kind': 'linear'}


def mixed_flow(dim, latent_dim=0, last=True, seed=0):
    """-> (NeuralFlow [coupling, ContinuousTanh, coupling, ContinuousActivation(torch.tanh)] (without its last layer: last=False) on
    the CPU, layer descriptions)."""
    torch.manual_seed(seed)
    descs = [coupling_desc(dim, 'ordered_left_half', latent_dim), {'kind': 'tanh', 'log_time': False},
             coupling_desc(dim, 'ordered_right_half', latent_dim), {'kind': 'act', 'name': 'tanh', 'temperature': 1.0}]
    if not last:
        descs = descs[:3]
    layers = []
    for d in descs:
        if d['kind'] == 'tanh':
            layers.append(st.ContinuousTanh(d['log_time']))
        elif d['kind'] == 'act':
            layers.append(st.ContinuousActivation(ACTS[d['name']], d['temperature']))
        else:
            layers.append(fd.build_transform(st, d))
    return st.NeuralFlow(layers), descs


def mixed_flow_eval(descs, state, x, t, t0=None, latent=None, dtype=torch.float64):
    """NeuralFlow.forward (flow.py:170-184) over `descs` in `dtype` on the CPU: the oracle's continuous_affine_coupling for the couplings,
    the restatements above for the rest."""
    state = {k: v.detach().cpu().to(dtype) for k, v in state.items()}
    x, t = x.detach().cpu().to(dtype), rows_like(t.detach().cpu().to(dtype), x)
    latent = None if latent is None else latent.detach().cpu().to(dtype)

    def step(i, d, x, tt, reverse):
        if d['kind'] == 'tanh':
            return tanh_flow(x, tt, d['log_time'], reverse)
        if d['kind'] == 'act':
            assert not reverse
            return mix(d['name'], x, tt, state[f'transforms.{i}.temperature'])
        return orc.continuous_affine_coupling(fd.transform_spec(d, state, f'transforms.{i}.'), x, tt, latent, reverse)[0]

    if t0 is not None:
        t0 = rows_like(t0.detach().cpu().to(dtype), x)
        for i in reversed(range(len(descs))):
            x = step(i, descs[i], x, t0, True)
    for i, d in enumerate(descs):
        x = step(i, d, x, t, False)
    return x
