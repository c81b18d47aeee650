#!/usr/bin/env python3
"""Capture the F22 golden vectors (ContinuousTransform with divergence='exact' over DiffeqExactTraceAttention on sets) from the
UNMODIFIED reference.

The recipe of make_golden_exact_set.py: it imports make_golden_cnf's module for the stubs (``torchtyping``, and this project's fixed-grid
``torchdiffeq`` stub -- the solver SPECIFICATION, DESIGN.md "CNF") ahead of the reference on ``sys.path``, no bytecode written, the
reference untouched.  The reference's own ``ContinuousTransform``, ``ODEfunc``, ``DiffeqExactTraceAttention``,
``DiffeqZeroTraceAttention``, ``MADE``, ``MLP``, ``attention`` and ``FuncAndDiagJac`` run on top of it.

    python tests/golden/make_golden_exact_attn.py

f22_exact_attn.npz:
  set/<shape>/h<n>/H<heads>/<solver>/T<T>/l<latent>   shapes (3,1,2) (5,3,2) (2,7,3) and the unbatched (6,2), hidden [16] / [12, 8],
                              d_h = 3, 1 / 2 / 4 heads, latent width 0 / 3, step_size 0.25, eval mode; per (shape, hidden, heads,
                              latent) two of the six solver x T combinations (euler | midpoint | rk4) x (1.0 | 0.7), dealt evenly.
                              x, latent, y / ldj (forward), x_back / ldj_back (the reverse solve from y), num_evals;
                              state/<key> for the q MADE's MASKS (its ordering and hidden degrees come from an unseeded numpy
                              generator); weights and biases are the default init under the case's seed, kept as sha256 per tensor in meta.
  bare/<name>/{state/<key>, x, latent, y, jac}   DiffeqZeroTraceAttention / DiffeqExactTraceAttention alone at t = 0.3, full state.
  meta                        `cases`, `bare`, `zero_trace_keys` / `exact_trace_keys` (the reference's state_dict key lists),
                              `signatures` (the reference constructors' parameter names and defaults).
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
D_H = 3
PAIRS = [(('euler', 1.0), ('rk4', 0.7)), (('midpoint', 1.0), ('euler', 0.7)), (('rk4', 1.0), ('midpoint', 0.7))]


def build(dim, hidden, latent, heads, T, solver, options):
    net = st.net.DiffeqExactTraceAttention(dim, hidden, dim, D_H, latent_dim=latent, n_heads=heads)
    return st.ContinuousTransform(dim, net=net, T=T, divergence='exact', has_latent=latent > 0, solver=solver, solver_options=options)


def f22():
    arrays, cases = {}, {}
    meta = {'signatures': {k: signature(getattr(st.net, k).__init__) for k in ('DiffeqZeroTraceAttention', 'DiffeqExactTraceAttention')}}
    seed, k = 2200, 0
    for shp in SHAPES:
        for hidden in ([16], [12, 8]):
            for heads in (1, 2, 4):
                if hidden[-1] % heads:
                    continue
                for latent in (0, 3):
                    pair = PAIRS[k % 3]
                    k += 1
                    for solver, T in pair:
                        dim = shp[-1]
                        case = f'set/{"x".join(map(str, shp))}/h{len(hidden)}/H{heads}/{solver}/T{T}/l{latent}'
                        options = {'step_size': 0.25}
                        seed += 1
                        torch.manual_seed(seed)
                        f = build(dim, hidden, latent, heads, T, solver, options).eval()
                        state = {n: v.clone() for n, v in f.state_dict().items()}
                        x = torch.randn(*shp)
                        lat = torch.randn(*shp[:-1], latent) if latent else None
                        arrays[f'{case}/x'] = x
                        if lat is not None:
                            arrays[f'{case}/latent'] = lat
                        for n, v in state.items():
                            if n.endswith('mask'):
                                arrays[f'{case}/state/{n}'] = v
                        n_evals = base.run(f, x, lat, arrays, case)
                        cases[case] = {'shape': list(shp), 'hidden': hidden, 'd_h': D_H, 'heads': heads, 'solver': solver,
                                       'options': options, 'T': T, 'latent': latent, 'seed': seed, 'num_evals': n_evals,
                                       'state_sha256': {n: base.sha(v) for n, v in state.items()
                                                        if n.endswith('weight') or n.endswith('bias')}}
    meta['cases'] = cases
    bare = {}
    t = torch.tensor([0.3])
    for name, kind, args, kw, shp, latent in (
            ('zero_default', 'DiffeqZeroTraceAttention', (3, [8, 6], 6), {'n_heads': 2}, (2, 5, 3), 0),
            ('zero_single', 'DiffeqZeroTraceAttention', (2, [8], 4), {'return_log_det_jac': False}, (3, 1, 2), 0),
            ('exact_default', 'DiffeqExactTraceAttention', (3, [8, 6], 3, 2), {'n_heads': 2}, (2, 5, 3), 0),
            ('exact_latent', 'DiffeqExactTraceAttention', (2, [8], 2, 4), {'latent_dim': 3, 'n_heads': 4}, (4, 2), 3)):
        seed += 1
        torch.manual_seed(seed)
        net = getattr(st.net, kind)(*args, **kw)
        x = torch.randn(*shp)
        lat = torch.randn(*shp[:-1], latent) if latent else None
        for n, v in net.state_dict().items():
            arrays[f'bare/{name}/state/{n}'] = v.clone()
        arrays[f'bare/{name}/x'] = x
        if lat is not None:
            arrays[f'bare/{name}/latent'] = lat
        with torch.no_grad():
            out = net(t, x, latent=lat) if kind == 'DiffeqExactTraceAttention' else net(t, x)
        if isinstance(out, tuple):
            arrays[f'bare/{name}/y'], arrays[f'bare/{name}/jac'] = out[0].detach(), out[1].detach()
        else:
            arrays[f'bare/{name}/y'] = out.detach()
        bare[name] = {'kind': kind, 'args': list(args), 'kwargs': kw, 'seed': seed, 'latent': latent, 'keys': list(net.state_dict()),
                      'state_sha256': {n: base.sha(v) for n, v in net.state_dict().items() if not n.endswith('mask')}}
    meta['bare'] = bare
    meta['zero_trace_keys'] = list(st.net.DiffeqZeroTraceAttention(2, [4, 6], 6, 2).state_dict())
    meta['exact_trace_keys'] = list(st.net.DiffeqExactTraceAttention(2, [4, 6], 2, 3, latent_dim=1, n_heads=2).state_dict())
    arrays = {n: base.npy(v) for n, v in arrays.items()}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'f22_exact_attn.npz')
    np.savez_compressed(path, **arrays)
    print(f'f22_exact_attn: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays, {len(cases)} cases')


if __name__ == '__main__':
    f22()
