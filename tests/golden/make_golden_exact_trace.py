#!/usr/bin/env python3
"""Capture the F17 golden vectors (ContinuousTransform with divergence='exact' over DiffeqExactTraceMLP) from the UNMODIFIED
reference.

The recipe of make_golden_cnf.py: stub modules ahead of the reference on ``sys.path`` (``torchtyping``, and this project's own
fixed-grid ``odeint`` as ``torchdiffeq`` -- the solver SPECIFICATION, taken from make_golden_cnf.py itself), no bytecode written, the
reference untouched.  The reference's own ``ContinuousTransform``, ``ODEfunc``, ``DiffeqExactTraceMLP``, ``MADE`` and
``FuncAndDiagJac`` run on top of it.

    python tests/golden/make_golden_exact_trace.py

f17_exact_trace.npz, per case `<name>`:
  <name>/state/<key>     the full state_dict (weights, biases, MASKS -- the hidden degrees come from an unseeded numpy generator, so
                         the masks cannot be rebuilt from a seed --, odefunc._num_evals)
  <name>/x, /latent      inputs;  /y, /ldj  forward;  /x_back, /ldj_back  the reverse solve from y
  <name>/bare_dy, /bare_jac   one bare DiffeqExactTraceMLP call at t = 0.3 on (x, latent)
  meta['cases'][<name>]  shape, hidden, d_h, latent, solver, options, T, seed, num_evals, keys (the state_dict's order),
                         state_sha256 (weights and biases under the seed: the host classes reproduce them draw for draw)
  meta['signatures']     the reference constructors' parameter names and defaults
"""
import inspect
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
_argv, sys.argv = sys.argv, [sys.argv[0]]
import make_golden_cnf as base  # noqa: E402  (imports the reference behind the stubs; its __main__ guard keeps it from capturing)
sys.argv = _argv

st = base.st
import numpy as np  # noqa: E402
import torch  # noqa: E402

# name: (shape, hidden, d_h, latent, solver, stepped, T)
CASES = {
    'a_10x2_h1_d3_rk4': ((10, 2), [32], 3, 0, 'rk4', 1, 1.0),
    'b_10x2_h2_d1_mid': ((10, 2), [64, 32], 1, 3, 'midpoint', 1, 0.7),
    'c_10x2_h1_d8_euler': ((10, 2), [32], 8, 3, 'euler', 0, 1.0),
    'd_70x1_h1_d3_rk4': ((70, 1), [32], 3, 3, 'rk4', 1, 0.7),
    'e_70x1_h2_d8_mid': ((70, 1), [64, 32], 8, 0, 'midpoint', 1, 1.0),
    'f_70x1_h2_d1_euler': ((70, 1), [64, 32], 1, 0, 'euler', 0, 0.7),
    'g_3x7x5_h1_d1_rk4': ((3, 7, 5), [32], 1, 0, 'rk4', 1, 1.0),
    'h_3x7x5_h2_d3_rk4': ((3, 7, 5), [64, 32], 3, 3, 'rk4', 1, 0.7),
    'i_3x7x5_h2_d8_mid': ((3, 7, 5), [64, 32], 8, 3, 'midpoint', 1, 1.0),
    'j_33x16_h1_d8_rk4': ((33, 16), [32], 8, 0, 'rk4', 1, 1.0),
    'k_33x16_h2_d3_rk4': ((33, 16), [64, 32], 3, 3, 'rk4', 1, 0.7),
    'l_33x16_h2_d1_euler': ((33, 16), [64, 32], 1, 3, 'euler', 0, 1.0),
}


def signature(fn):
    return {k: (None if p.default is inspect.Parameter.empty else repr(p.default)) for k, p in inspect.signature(fn).parameters.items()
            if k != 'self'}


def f17():
    arrays, cases = {}, {}
    meta = {'signatures': {'MADE': signature(st.net.MADE.__init__), 'DiffeqZeroTraceMLP': signature(st.net.DiffeqZeroTraceMLP.__init__),
                           'DiffeqExactTrace': signature(st.net.DiffeqExactTrace.__init__),
                           'DiffeqExactTraceMLP': signature(st.net.DiffeqExactTraceMLP.__init__)}}
    seed = 1700
    for case, (shp, hidden, d_h, latent, solver, stepped, T) in CASES.items():
        dim = shp[-1]
        options = {'step_size': 0.25} if stepped else {}
        seed += 1
        torch.manual_seed(seed)
        net = st.net.DiffeqExactTraceMLP(dim, hidden, dim, d_h, latent_dim=latent)
        f = st.ContinuousTransform(dim, net=net, T=T, divergence='exact', has_latent=latent > 0, solver=solver,
                                   solver_options=options).eval()
        state = {k: v.clone() for k, v in f.state_dict().items()}
        x = torch.randn(*shp)
        lat = torch.randn(*shp[:-1], latent) if latent else None
        arrays[f'{case}/x'] = x
        if lat is not None:
            arrays[f'{case}/latent'] = lat
        for k, v in state.items():
            arrays[f'{case}/state/{k}'] = v
        dy, jac = net(torch.tensor([0.3]), x, latent=lat)
        arrays[f'{case}/bare_dy'], arrays[f'{case}/bare_jac'] = dy.detach(), jac.detach()
        n = base.run(f, x, lat, arrays, case)
        cases[case] = {'shape': list(shp), 'hidden': hidden, 'd_h': d_h, 'latent': latent, 'solver': solver, 'options': options, 'T': T,
                       'seed': seed, 'num_evals': n, 'keys': list(state),
                       'state_sha256': {k: base.sha(v) for k, v in state.items() if k.endswith('weight') or k.endswith('bias')}}
    meta['cases'] = cases
    arrays = {k: base.npy(v) for k, v in arrays.items()}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'f17_exact_trace.npz')
    np.savez_compressed(path, **arrays)
    print(f'f17_exact_trace: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays, {len(cases)} cases')


if __name__ == '__main__':
    f17()
