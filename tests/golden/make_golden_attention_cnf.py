#!/usr/bin/env python3
"""Capture the F20 golden vectors (ContinuousTransform over sets with DiffeqSelfAttention under set_data=True /
divergence='compute_set') from the UNMODIFIED reference.

The recipe of make_golden_set_cnf.py: it imports make_golden_cnf's module for the stubs (``torchtyping``, and this project's fixed-grid
``torchdiffeq`` stub -- the solver SPECIFICATION, DESIGN.md "CNF") ahead of the reference on ``sys.path``, no bytecode written, the
reference untouched.  The reference's own ``ContinuousTransform``, ``ODEfunc``, ``DiffeqSelfAttention``, ``SelfAttention``,
``safe_softmax`` and ``divergence_exact_for_sets`` run on top of it.

    python tests/golden/make_golden_attention_cnf.py

f20_attention_cnf.npz:
  set/<shape>/h<n>/n<heads>/m<0|1>/<solver>/T<T>/l<latent>   shapes (3,1,2) (5,3,2) (2,7,3) and the unbatched (6,2), hidden_dim [8] /
                              [12, 8], n_heads 1 / 2, mask_diagonal off / on, latent width 0 / 3, step_size 0.25, eval mode; per
                              (shape, hidden_dim, n_heads, mask_diagonal, latent) two of the six solver x T combinations (euler |
                              midpoint | rk4) x (1.0 | 0.7), dealt evenly.  x, latent, y / ldj (forward), x_back / ldj_back (the reverse
                              solve from y), num_evals; the weights are the default init under the case's seed, kept as sha256 per
                              tensor in meta.
  bare/<name>/{state/<key>, x, latent, dy, div}   DiffeqSelfAttention alone at t = 0.3, full state; div = divergence_exact_for_sets.
  meta                        `cases`, `bare`, `keys` (the reference's state_dict key list), `signature` (the reference constructor's
                              parameter names and defaults).
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
_argv, sys.argv = sys.argv, [sys.argv[0]]
import make_golden_cnf as base  # noqa: E402  (imports the reference over the stubs)
from make_golden_exact_trace import signature  # noqa: E402
sys.argv = _argv

import numpy as np  # noqa: E402
import torch  # noqa: E402

st = base.st
SHAPES = [(3, 1, 2), (5, 3, 2), (2, 7, 3), (6, 2)]
PAIRS = [(('euler', 1.0), ('rk4', 0.7)), (('midpoint', 1.0), ('euler', 0.7)), (('rk4', 1.0), ('midpoint', 0.7))]


def build(dim, hidden, latent, n_heads, mask_diagonal, T, solver, options):
    net = st.net.DiffeqSelfAttention(dim + 1 + latent, hidden, dim, n_heads=n_heads, mask_diagonal=mask_diagonal)
    return st.ContinuousTransform(dim, net=net, T=T, divergence='compute_set', has_latent=latent > 0, solver=solver,
                                  solver_options=options, set_data=True)


def f20():
    arrays, cases = {}, {}
    meta = {'signature': signature(st.net.DiffeqSelfAttention.__init__)}
    seed, k = 2000, 0
    for shp in SHAPES:
        for hidden in ([8], [12, 8]):
            for n_heads in (1, 2):
                for md in (False, True):
                    for latent in (0, 3):
                        pair = PAIRS[k % 3]
                        k += 1
                        for solver, T in pair:
                            dim = shp[-1]
                            case = f'set/{"x".join(map(str, shp))}/h{len(hidden)}/n{n_heads}/m{int(md)}/{solver}/T{T}/l{latent}'
                            options = {'step_size': 0.25}
                            seed += 1
                            torch.manual_seed(seed)
                            f = build(dim, hidden, latent, n_heads, md, T, solver, options).eval()
                            state = {n: v.clone() for n, v in f.state_dict().items()}
                            x = torch.randn(*shp)
                            lat = torch.randn(*shp[:-1], latent) if latent else None
                            arrays[f'{case}/x'] = x
                            if lat is not None:
                                arrays[f'{case}/latent'] = lat
                            n_evals = base.run(f, x, lat, arrays, case)
                            cases[case] = {'shape': list(shp), 'hidden': hidden, 'n_heads': n_heads, 'mask_diagonal': md, 'solver': solver,
                                           'options': options, 'T': T, 'latent': latent, 'seed': seed, 'num_evals': n_evals,
                                           'state_sha256': {n: base.sha(v) for n, v in state.items()
                                                            if n.endswith('weight') or n.endswith('bias')}}
    meta['cases'] = cases
    bare = {}
    t = torch.tensor([0.3])
    for name, args, kw, shp, latent in (
            ('single', (3, [8], 2), {}, (2, 5, 2), 0),
            ('deep_heads', (4, [12, 8], 3), {'n_heads': 4}, (3, 4, 3), 0),
            ('masked_latent', (6, [12, 8], 2), {'n_heads': 2, 'mask_diagonal': True}, (2, 6, 2), 3),
            ('one_masked', (3, [8], 2), {'n_heads': 2, 'mask_diagonal': True}, (4, 1, 2), 0),
            ('one', (6, [12, 8], 3), {}, (1, 3), 2),
            ('unbatched', (4, [8], 3), {'n_heads': 2}, (6, 3), 0)):
        seed += 1
        torch.manual_seed(seed)
        net = st.net.DiffeqSelfAttention(*args, **kw)
        x = torch.randn(*shp)
        lat = torch.randn(*shp[:-1], latent) if latent else None
        for n, v in net.state_dict().items():
            arrays[f'bare/{name}/state/{n}'] = v.clone()
        arrays[f'bare/{name}/x'] = x
        if lat is not None:
            arrays[f'bare/{name}/latent'] = lat
        xx = x.clone().requires_grad_(True)
        dy = net(t, xx, latent=lat)
        div = st.util.divergence_exact_for_sets(dy, xx)
        arrays[f'bare/{name}/dy'], arrays[f'bare/{name}/div'] = dy.detach(), div.detach()
        bare[name] = {'args': list(args), 'kwargs': kw, 'seed': seed, 'latent': latent, 'keys': list(net.state_dict())}
    meta['bare'] = bare
    meta['keys'] = list(st.net.DiffeqSelfAttention(3, [4, 6], 2, n_heads=2).state_dict())
    arrays = {n: base.npy(v) for n, v in arrays.items()}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'f20_attention_cnf.npz')
    np.savez_compressed(path, **arrays)
    print(f'f20_attention_cnf: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays, {len(cases)} cases')


if __name__ == '__main__':
    f20()
