#!/usr/bin/env python3
"""Capture the F16 golden vectors (ContinuousTransform, stribor/flows/cnf.py) from the UNMODIFIED reference.

The recipe of make_golden_iresnet.py (stub modules ahead of the reference on ``sys.path``, no bytecode written, the reference
untouched) with one difference: the ``torchdiffeq`` stub is this project's own small fixed-grid ``odeint`` -- tuple state, the
solvers euler / midpoint / rk4 (3/8 rule) and the ``step_size`` grid, restating torchdiffeq 0.2.2's fixed-grid family (that
package is not installed where the fixtures are made; DESIGN.md "CNF").  This stub is the SPECIFICATION the kernel is held to.
The reference's own ``ContinuousTransform``, ``ODEfunc``, ``DiffeqMLP`` and ``divergence_exact`` run on top of it.

    python tests/golden/make_golden_cnf.py

f16_cnf.npz:
  grid/<shape>/h<n>/<solver>/s<0|1>/T<T>/l<latent>   shapes (10,2) (2,10) (7,4,5), hidden [64] / [32, 32], each solver with
                              step_size 0.25 (s1) and without (s0), T in {1.0, 0.7}, latent width 0 / 3, eval mode (exact divergence):
                              the state is the default init under the case's seed, kept as sha256 per tensor in meta (the host classes
                              reproduce it draw for draw); x, latent, y / ldj (forward), x_back /
                              ldj_back (the reverse solve from y), num_evals.
  kernel                      dim 32, [128, 128], N = 256, rk4 at 16 steps: state as sha256 only, x regenerated from the seed.
  meta                        per case: shape, hidden, solver, options, T, latent, seed; `signature`: the reference constructor's
                              parameter names and defaults.
"""
import hashlib
import inspect
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'

ODEINT_STUB = '''
"""Fixed-grid odeint on tuple states: euler, midpoint, rk4 (the 3/8 rule), options={'step_size': h}."""
import torch


def _grid(t, step_size):
    t0, t1 = t[0], t[-1]
    if step_size is None:
        return torch.stack([t0, t1])
    sgn = -1.0 if t1 < t0 else 1.0
    n = int(torch.ceil((t1 - t0).abs() / step_size + 1).item())
    g = t0 + sgn * (torch.arange(0, n).to(t) * step_size)
    g[-1] = t1
    return g


def _step(func, method, t0, t1, y):
    dt = t1 - t0
    k1 = func(t0, y)
    if method == 'euler':
        return tuple(dt * k for k in k1)
    if method == 'midpoint':
        half = 0.5 * dt
        k2 = func(t0 + half, tuple(a + k * half for a, k in zip(y, k1)))
        return tuple(dt * k for k in k2)
    third, two_thirds = 1.0 / 3.0, 2.0 / 3.0
    k2 = func(t0 + dt * third, tuple(a + dt * k * third for a, k in zip(y, k1)))
    k3 = func(t0 + dt * two_thirds, tuple(a + dt * (b - k * third) for a, k, b in zip(y, k1, k2)))
    k4 = func(t1, tuple(a + dt * (k - b + c) for a, k, b, c in zip(y, k1, k2, k3)))
    return tuple((k + 3 * (b + c) + d) * dt * 0.125 for k, b, c, d in zip(k1, k2, k3, k4))


def odeint(func, y0, t, *, rtol=1e-7, atol=1e-9, method=None, options=None, **unused):
    if method not in ('euler', 'midpoint', 'rk4'):
        raise NotImplementedError(method)
    assert len(t) == 2
    grid = _grid(t, (options or {}).get('step_size'))
    y = tuple(y0)
    for i in range(len(grid) - 1):
        inc = _step(func, method, grid[i], grid[i + 1], y)
        y = tuple(a + b for a, b in zip(y, inc))
    return tuple(torch.stack([a, b]) for a, b in zip(y0, y))


odeint_adjoint = odeint
'''


def import_reference():
    stub = tempfile.mkdtemp(prefix='stribor_cnf_stubs_')
    os.makedirs(os.path.join(stub, 'torchtyping'))
    os.makedirs(os.path.join(stub, 'torchdiffeq'))
    with open(os.path.join(stub, 'torchtyping', '__init__.py'), 'w') as f:
        f.write('class TensorType:\n    def __class_getitem__(cls, item):\n        return cls\n')
    with open(os.path.join(stub, 'torchdiffeq', '__init__.py'), 'w') as f:
        f.write(ODEINT_STUB)
    sys.path.insert(0, REF)
    sys.path.insert(0, stub)
    import stribor  # noqa
    assert stribor.__file__.startswith(REF), stribor.__file__
    return stribor


st = import_reference()

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)
SHAPES = [(10, 2), (2, 10), (7, 4, 5)]


def npy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def sha(t):
    a = np.ascontiguousarray(npy(t))
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def build(dim, hidden, latent, T, solver, options):
    return st.ContinuousTransform(dim, net=st.net.DiffeqMLP(dim + 1 + latent, hidden, dim), T=T, divergence='approximate',
                                  has_latent=latent > 0, solver=solver, solver_options=options)


def run(f, x, latent, arrays, case):
    kw = {} if latent is None else {'latent': latent}
    y, ldj = f.forward_and_log_det_jacobian(x, **kw)
    arrays[f'{case}/y'], arrays[f'{case}/ldj'] = y.detach(), ldj.detach()
    n1 = f._num_evals()
    xb, ldjb = f.inverse_and_log_det_jacobian(y.detach(), **kw)
    arrays[f'{case}/x_back'], arrays[f'{case}/ldj_back'] = xb.detach(), ldjb.detach()
    assert f._num_evals() == n1
    return int(n1)


def f16():
    arrays, meta = {}, {}
    sig = inspect.signature(st.ContinuousTransform.__init__)
    meta['signature'] = {k: (None if p.default is inspect.Parameter.empty else repr(p.default)) for k, p in sig.parameters.items()
                         if k != 'self'}
    cases = {}
    seed = 1600
    for shp in SHAPES:
        for hidden in ([64], [32, 32]):
            for solver in ('euler', 'midpoint', 'rk4'):
                for stepped in (0, 1):
                    for T in (1.0, 0.7):
                        for latent in (0, 3):
                            dim = shp[-1]
                            case = f'grid/{"x".join(map(str, shp))}/h{len(hidden)}/{solver}/s{stepped}/T{T}/l{latent}'
                            options = {'step_size': 0.25} if stepped else {}
                            seed += 1
                            torch.manual_seed(seed)
                            f = build(dim, hidden, latent, T, solver, options).eval()
                            state = {k: v.clone() for k, v in f.state_dict().items()}
                            x = torch.randn(*shp)
                            lat = torch.randn(*shp[:-1], latent) if latent else None
                            arrays[f'{case}/x'] = x
                            if lat is not None:
                                arrays[f'{case}/latent'] = lat
                            n = run(f, x, lat, arrays, case)
                            cases[case] = {'shape': list(shp), 'hidden': hidden, 'solver': solver, 'options': options, 'T': T,
                                           'latent': latent, 'seed': seed, 'num_evals': n,
                                           'state_sha256': {k: sha(v) for k, v in state.items()}}
    # the kernel-sized case: the weights are the default init under the seed (held to their hashes), x from the seed
    dim, hidden, seed = 32, [128, 128], 1699
    torch.manual_seed(seed)
    f = build(dim, hidden, 0, 1.0, 'rk4', {'step_size': 1.0 / 16}).eval()
    state = {k: v.clone() for k, v in f.state_dict().items()}
    torch.manual_seed(seed + 1)
    x = torch.randn(256, dim)
    n = run(f, x, None, arrays, 'kernel')
    cases['kernel'] = {'shape': [256, dim], 'hidden': hidden, 'solver': 'rk4', 'options': {'step_size': 1.0 / 16}, 'T': 1.0,
                       'latent': 0, 'seed': seed, 'num_evals': n, 'state_sha256': {k: sha(v) for k, v in state.items()}}
    meta['cases'] = cases
    arrays = {k: npy(v) for k, v in arrays.items()}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'f16_cnf.npz')
    np.savez_compressed(path, **arrays)
    print(f'f16_cnf: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays, {len(cases)} cases')


if __name__ == '__main__':
    f16()
