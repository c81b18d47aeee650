#!/usr/bin/env python3
"""Capture the F18 golden vectors (ContinuousTransform over sets: DiffeqDeepset / EquivariantNet with set_data=True) from the
UNMODIFIED reference.

The recipe of make_golden_cnf.py, whose module this one imports for it: stub ``torchtyping`` and this project's fixed-grid
``torchdiffeq`` stub (the solver SPECIFICATION, DESIGN.md "CNF") ahead of the reference on ``sys.path``, no bytecode written, the
reference untouched.  The reference's own ``ContinuousTransform``, ``ODEfunc``, ``DiffeqDeepset``, ``EquivariantNet`` and
``divergence_exact_for_sets`` run on top of it.

    python tests/golden/make_golden_set_cnf.py

f18_set_cnf.npz:
  set/<B>x<N>x<dim>/h<n>/<solver>/T<T>/l<latent>   shapes (3,1,2) (5,3,2) (2,7,3), hidden [16] / [12, 20], each solver at step_size
                              0.25, T in {1.0, 0.7}, latent width 0 / 3, set_data=True, divergence='compute', eval mode: the state is
                              the default init under the case's seed, kept as sha256 per tensor in meta; x, latent, y / ldj (forward),
                              x_back / ldj_back (the reverse solve from y), num_evals.
  net/<name>/{x, mask, y, y_masked}   EquivariantNet alone, with and without a mask (..., N, 1); state as sha256 in meta.
  meta                        `cases` (shape, hidden, solver, options, T, latent, seed, num_evals, state_sha256), `nets` (args, seed,
                              state_sha256), `net_keys` / `deepset_keys`: the reference's state_dict key lists.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_cnf as base  # noqa: E402  (imports the reference over the stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

st = base.st
SHAPES = [(3, 1, 2), (5, 3, 2), (2, 7, 3)]


def build(dim, hidden, latent, T, solver, options):
    return st.ContinuousTransform(dim, net=st.net.DiffeqDeepset(dim + 1 + latent, hidden, dim), T=T, divergence='compute',
                                  has_latent=latent > 0, solver=solver, solver_options=options, set_data=True)


def f18():
    arrays, meta, cases = {}, {}, {}
    seed = 1800
    for shp in SHAPES:
        for hidden in ([16], [12, 20]):
            for solver in ('euler', 'midpoint', 'rk4'):
                for T in (1.0, 0.7):
                    for latent in (0, 3):
                        dim = shp[-1]
                        case = f'set/{"x".join(map(str, shp))}/h{len(hidden)}/{solver}/T{T}/l{latent}'
                        options = {'step_size': 0.25}
                        seed += 1
                        torch.manual_seed(seed)
                        f = build(dim, hidden, latent, T, solver, options).eval()
                        state = {k: v.clone() for k, v in f.state_dict().items()}
                        x = torch.randn(*shp)
                        lat = torch.randn(*shp[:-1], latent) if latent else None
                        arrays[f'{case}/x'] = x
                        if lat is not None:
                            arrays[f'{case}/latent'] = lat
                        n = base.run(f, x, lat, arrays, case)
                        cases[case] = {'shape': list(shp), 'hidden': hidden, 'solver': solver, 'options': options, 'T': T,
                                       'latent': latent, 'seed': seed, 'num_evals': n,
                                       'state_sha256': {k: base.sha(v) for k, v in state.items()}}
    meta['cases'] = cases
    meta['deepset_keys'] = list(build(2, [4, 5], 0, 1.0, 'rk4', {}).state_dict())
    nets = {}
    for name, args, kw, shp in (('tanh', (4, [6, 5], 3), {}, (2, 5, 4)), ('relu_final', (3, [7], 2), {'activation': 'ReLU', 'final_activation': 'Tanh'}, (4, 3)),
                                ('single', (2, [5, 5], 2), {'activation': 'ELU'}, (3, 1, 2))):
        seed += 1
        torch.manual_seed(seed)
        net = st.net.EquivariantNet(*args, **kw)
        x = torch.randn(*shp)
        mask = (torch.rand(*shp[:-1], 1) > 0.4).float()
        mask[..., 0, :] = 1                                     # (an all-masked set divides by zero in the reference)
        with torch.no_grad():
            arrays[f'net/{name}/x'], arrays[f'net/{name}/mask'] = x, mask
            arrays[f'net/{name}/y'] = net(x, None)
            arrays[f'net/{name}/y_masked'] = net(x, mask)
        nets[name] = {'args': list(args), 'kwargs': kw, 'seed': seed, 'state_sha256': {k: base.sha(v) for k, v in net.state_dict().items()}}
    meta['net_keys'] = list(st.net.EquivariantNet(4, [6, 5], 3).state_dict())
    meta['nets'] = nets
    arrays = {k: base.npy(v) for k, v in arrays.items()}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'f18_set_cnf.npz')
    np.savez_compressed(path, **arrays)
    print(f'f18_set_cnf: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays, {len(cases)} cases')


if __name__ == '__main__':
    f18()
