"""Helpers of the base-density tests (test_base_host.py, test_gpu_base.py): the F21 cases rebuilt through the host classes, and the
torch.distributions objects that serve as truth (fp64, CPU) and as the reference whose fp32 error sets the bound (cnfhelp.bound)."""
import torch
import torch.distributions as td

import stribor_amd as st
from goldens import Golden
from stribor_amd.util import flowdesc as fd

_G = None


def golden():
    global _G
    if _G is None:
        _G = Golden('f21_base')
    return _G


def f21_cases():
    """-> {name: (make() -> st distribution on the CPU, x, lp32, lp64, exact)}; exact: the closed form's op sequence is torch's own,
    so its fp32 values equal the fixture's bit for bit (the multivariate normal derives its factor in fp64 and is held to a bound)."""
    g = golden().t
    cases = {'normal_float': (lambda: st.Normal(0.5, 2.0), g('normal_float/x'), g('normal_float/lp32'), g('normal_float/lp64'), True)}
    nv = lambda: st.Normal(g('normal_vec/loc'), g('normal_vec/scale'))
    cases['normal_vec'] = (nv, g('normal_vec/x'), g('normal_vec/lp32'), g('normal_vec/lp64'), True)
    cases['normal_vec_3'] = (nv, g('normal_vec/x3'), g('normal_vec/lp32_3'), g('normal_vec/lp64_3'), True)
    cases['unit_uniform'] = (lambda: st.UnitUniform(3), g('unit_uniform/x'), g('unit_uniform/lp32'), g('unit_uniform/lp64'), True)
    cases['uniform_vec'] = (lambda: st.Uniform(g('uniform_vec/low'), g('uniform_vec/high')), g('uniform_vec/x'), g('uniform_vec/lp32'),
                            g('uniform_vec/lp64'), True)
    cases['uniform_out'] = (lambda: st.Uniform(g('uniform_vec/low'), g('uniform_vec/high'), validate_args=False), g('uniform_out/x'),
                            g('uniform_out/lp32'), g('uniform_out/lp64'), True)
    for form, kw in (('cov', 'covariance_matrix'), ('prec', 'precision_matrix'), ('tril', 'scale_tril')):
        cases[f'mvn_{form}'] = ((lambda form=form, kw=kw: st.MultivariateNormal(g('mvn/loc'), **{kw: g(f'mvn/{form}')})), g('mvn/x'),
                                g(f'mvn/lp32_{form}'), g(f'mvn/lp64_{form}'), False)
    return cases


FLOW_BASES = ('normal', 'mvn', 'uniform')


def f21_base(name):
    g = golden().t
    if name == 'normal':
        return st.Normal(g('flow/normal/loc'), g('flow/normal/scale'))
    if name == 'mvn':
        return st.MultivariateNormal(g('flow/mvn/loc'), scale_tril=g('flow/mvn/tril'))
    return st.Uniform(g('flow/uniform/low'), g('flow/uniform/high'))


def f21_flow(name):
    """-> (flow on the CPU with the fixture's state, desc, x [9, 6], lp32, lp64)"""
    G = golden()
    desc = G.meta['flow_desc']
    flow = st.NormalizingFlow(f21_base(name), [fd.build_transform(st, d) for d in desc])
    missing, unexpected = flow.load_state_dict(G.state('flow'), strict=False)
    assert not unexpected and all(k.startswith('base_dist.') for k in missing), (missing, unexpected)
    return flow, desc, G.t('flow/x'), G.t(f'flow/{name}/lp32'), G.t(f'flow/{name}/lp64')


def torch_dist(d, dtype=torch.float64, device='cpu'):
    """The torch.distributions object of an st distribution, parameters cast to dtype on device (validate_args=False: the sample is
    never validated here either)."""
    c = lambda t: t.detach().to(device=device, dtype=dtype)
    if isinstance(d, st.MultivariateNormal):
        return td.MultivariateNormal(c(d.loc), validate_args=False, **{d._matrix_name: c(d._matrix)})
    if isinstance(d, st.Normal):
        base = td.Normal(c(d.loc), c(d.scale), validate_args=False)
    else:
        base = td.Uniform(c(d.low), c(d.high), validate_args=False)
    return base if d.elementwise else td.Independent(base, 1)


def well_conditioned_tril(D, gen):
    """A lower-triangular factor with its diagonal in [0.5, 2] and off-diagonal entries 0.1 * randn / sqrt(D)."""
    L = torch.tril(torch.randn(D, D, generator=gen) * (0.1 / D ** 0.5), -1)
    return L + torch.diag(0.5 + 1.5 * torch.rand(D, generator=gen))
