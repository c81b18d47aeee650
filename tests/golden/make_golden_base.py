#!/usr/bin/env python3
"""Capture the F21 golden vectors (base densities: stribor/dist/normal.py, dist/uniform.py) from the UNMODIFIED reference.

The recipe of make_golden.py: annotation-only stub modules (``torchtyping``, ``torchdiffeq``) ahead of the reference on ``sys.path``,
no bytecode written, the reference untouched.  The fixture holds data only: inputs, the reference's fp32 values and its fp64 values
(the same objects built from ``.double()`` parameters on ``.double()`` inputs).

    python tests/golden/make_golden_base.py <path of the reference checkout>

f21_base.npz:
  normal_float/{x, lp32, lp64}              Normal(0.5, 2.0), element-wise, on [5, 3]
  normal_vec/{loc, scale, x, lp32, lp64, x3, lp32_3, lp64_3}   D = 5 on [7, 5] and [2, 3, 5]
  unit_uniform/{x, lp32, lp64}              UnitUniform(3), in-support samples, x[0, 0] == low
  uniform_vec/{low, high, x, lp32, lp64}    D = 4, in-support samples, x[0, 1] == low
  uniform_out/{x, lp32, lp64}               the same bounds, validate_args=False: x[1, 2] == high, x[3, 0] below low, x[4, 3] above high
  mvn/{loc, cov, prec, tril, x, lp32_<form>, lp64_<form>}      D = 4, form in cov | prec | tril (one covariance)
  flow/state/<k>, flow/x                    NormalizingFlow(base, [2 affine couplings, D = 6, hidden 8]) on [9, 6]
  flow/<base>/{lp32, lp64} + its parameters base in normal | mvn | uniform (wide: every latent inside)
  meta                                      seeds, the flow's description
"""
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))          # repo root: flowdesc lives in stribor_amd.util
REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('STRIBOR_REFERENCE', ''))


def import_reference():
    stub = tempfile.mkdtemp(prefix='stribor_base_stubs_')
    for name, body in (('torchtyping', 'class TensorType:\n    def __class_getitem__(cls, item):\n        return cls\n'),
                       ('torchdiffeq', 'def odeint(*a, **k):\n    raise NotImplementedError\n\n\nodeint_adjoint = odeint\n')):
        os.makedirs(os.path.join(stub, name))
        with open(os.path.join(stub, name, '__init__.py'), 'w') as f:
            f.write(body)
    sys.path.insert(0, REF)
    sys.path.insert(0, stub)
    import stribor  # noqa
    assert stribor.__file__.startswith(REF), stribor.__file__
    return stribor


ref = import_reference()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stribor_amd.util import flowdesc as fd  # noqa: E402

SEED = 2100
FLOW_DESC = [{'kind': 'coupling_affine', 'dim': 6, 'hidden': [8], 'mask': 'ordered_right_half' if i % 2 == 0 else 'ordered_left_half',
              'latent_dim': 0} for i in range(2)]


def d64(t):
    return t.double() if torch.is_tensor(t) else t


def both(arrays, key, make, x, suffix=''):
    """make(cast) -> the reference distribution from parameters passed through `cast`; records its fp32 and fp64 log_prob of x."""
    with torch.no_grad():
        arrays[f'{key}/lp32{suffix}'] = make(lambda t: t).log_prob(x)
        arrays[f'{key}/lp64{suffix}'] = make(d64).log_prob(x.double())
    assert arrays[f'{key}/lp32{suffix}'].dtype == torch.float32 and arrays[f'{key}/lp64{suffix}'].dtype == torch.float64


def f21():
    arrays, meta = {}, {'seed': SEED, 'flow_desc': FLOW_DESC}
    torch.manual_seed(SEED)

    x = torch.randn(5, 3) * 2
    arrays['normal_float/x'] = x
    with torch.no_grad():
        arrays['normal_float/lp32'] = ref.Normal(0.5, 2.0).log_prob(x)
        torch.set_default_dtype(torch.float64)          # (float parameters become tensors of the default dtype)
        arrays['normal_float/lp64'] = ref.Normal(0.5, 2.0).log_prob(x.double())
        torch.set_default_dtype(torch.float32)
    assert arrays['normal_float/lp32'].shape == (5, 3) and arrays['normal_float/lp64'].dtype == torch.float64

    loc, scale = torch.randn(5), torch.rand(5) * 1.5 + 0.5
    x, x3 = torch.randn(7, 5) * 2, torch.randn(2, 3, 5) * 2
    arrays.update({'normal_vec/loc': loc, 'normal_vec/scale': scale, 'normal_vec/x': x, 'normal_vec/x3': x3})
    both(arrays, 'normal_vec', lambda c: ref.Normal(c(loc), c(scale)), x)
    both(arrays, 'normal_vec', lambda c: ref.Normal(c(loc), c(scale)), x3, '_3')

    x = torch.rand(6, 3)
    x[0, 0] = 0.0
    arrays['unit_uniform/x'] = x
    with torch.no_grad():
        arrays['unit_uniform/lp32'] = ref.UnitUniform(3).log_prob(x)
        u = ref.UnitUniform(3)
        arrays['unit_uniform/lp64'] = ref.Uniform(u.low.double(), u.high.double()).log_prob(x.double())

    low, high = torch.tensor([0.0, -1.5, 2.0, -0.25]), torch.tensor([1.0, 1.0, 5.0, 0.75])
    x = low + torch.rand(6, 4) * (high - low) * 0.999
    x[0, 1] = low[1]
    arrays.update({'uniform_vec/low': low, 'uniform_vec/high': high, 'uniform_vec/x': x})
    both(arrays, 'uniform_vec', lambda c: ref.Uniform(c(low), c(high)), x)
    xo = x.clone()
    xo[1, 2] = high[2]
    xo[3, 0] = low[0] - 0.5
    xo[4, 3] = high[3] + 1.0
    arrays['uniform_out/x'] = xo
    both(arrays, 'uniform_out', lambda c: ref.Uniform(c(low), c(high), validate_args=False), xo)
    lp = arrays['uniform_out/lp32']
    assert torch.isinf(lp[[1, 3, 4]]).all() and torch.isfinite(lp[[0, 2, 5]]).all()

    a = torch.randn(4, 4)
    cov = a @ a.T / 4 + torch.eye(4)
    cov = (cov + cov.T) / 2
    forms = {'cov': ('covariance_matrix', cov), 'prec': ('precision_matrix', torch.linalg.inv(cov.double()).float()),
             'tril': ('scale_tril', torch.linalg.cholesky(cov.double()).float())}
    forms['prec'] = ('precision_matrix', (forms['prec'][1] + forms['prec'][1].T) / 2)
    loc, x = torch.randn(4), torch.randn(8, 4) * 1.5
    arrays.update({'mvn/loc': loc, 'mvn/x': x, **{f'mvn/{k}': m for k, (_, m) in forms.items()}})
    for k, (kw, m) in forms.items():
        both(arrays, 'mvn', lambda c: ref.MultivariateNormal(c(loc), **{kw: c(m)}), x, f'_{k}')

    # flows: the transforms are the reference's default init under the seed; one state for the three bases
    torch.manual_seed(SEED + 1)
    transforms = [fd.build_transform(ref, d) for d in FLOW_DESC]
    y = torch.randn(9, 6)
    arrays['flow/x'] = y
    n_loc, n_scale = torch.randn(6) * 0.5, torch.rand(6) + 0.5
    b = torch.randn(6, 6) * 0.2
    m_tril = torch.tril(b, -1) + torch.diag(torch.rand(6) + 0.5)
    m_loc = torch.randn(6) * 0.5
    u_low, u_high = torch.full((6,), -50.0), torch.linspace(40.0, 60.0, 6)
    arrays.update({'flow/normal/loc': n_loc, 'flow/normal/scale': n_scale, 'flow/mvn/loc': m_loc, 'flow/mvn/tril': m_tril,
                   'flow/uniform/low': u_low, 'flow/uniform/high': u_high})
    bases = {'normal': lambda c: ref.Normal(c(n_loc), c(n_scale)), 'mvn': lambda c: ref.MultivariateNormal(c(m_loc), scale_tril=c(m_tril)),
             'uniform': lambda c: ref.Uniform(c(u_low), c(u_high))}
    flow = ref.NormalizingFlow(bases['normal'](lambda t: t), transforms)
    for k, v in flow.state_dict().items():
        arrays[f'flow/state/{k}'] = v.clone()
    for name, make in bases.items():
        with torch.no_grad():
            arrays[f'flow/{name}/lp32'] = ref.NormalizingFlow(make(lambda t: t), transforms).log_prob(y)
    for t in transforms:
        t.double()
    for name, make in bases.items():
        with torch.no_grad():
            arrays[f'flow/{name}/lp64'] = ref.NormalizingFlow(make(d64), transforms).log_prob(y.double())
        assert arrays[f'flow/{name}/lp32'].shape == (9, 1) and torch.isfinite(arrays[f'flow/{name}/lp64']).all()

    arrays = {k: v.detach().cpu().numpy() for k, v in arrays.items()}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'f21_base.npz')
    np.savez_compressed(path, **arrays)
    print(f'f21_base: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays')


if __name__ == '__main__':
    f21()
