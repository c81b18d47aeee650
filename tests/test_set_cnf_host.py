"""CPU: host logic of the set CNF -- EquivariantLayer / EquivariantNet / DiffeqDeepset against fixture F18 (captured from the
reference), the closed-form set divergence against fp64 autograd, the composition path, and sx_cnf_set_flow's coverage gate."""
import pytest
import torch

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.flows import cnf

import cnfhelp as ch
import sethelp as sh

ACTS = ['Identity', 'Tanh', 'ReLU', 'Sigmoid', 'ELU', 'Softplus', 'LeakyReLU']


def test_set_nets_are_exported():
    assert issubclass(st.net.DiffeqDeepset, st.net.DiffeqConcat)
    net = st.net.DiffeqDeepset(3, [64, 64], 2)
    assert type(net.net) is st.net.EquivariantNet and type(net.net.layers[0]) is st.net.EquivariantLayer
    st.ContinuousTransform(2, net=net, set_data=True)          # the reference user's line of the issue


def test_state_dict_keys_match_reference():
    g = sh.golden()
    assert list(st.net.EquivariantNet(4, [6, 5], 3).state_dict()) == g.meta['net_keys']
    f = st.ContinuousTransform(2, net=st.net.DiffeqDeepset(3, [4, 5], 2), T=1.0, divergence='compute', solver='rk4', solver_options={},
                               set_data=True)
    assert list(f.state_dict()) == g.meta['deepset_keys']


@pytest.mark.parametrize('case', [c for c in sh.case_names() if '/euler/T1.0/' in c])
def test_default_init_matches_reference_draw_for_draw(case):
    f, _, _, m = sh.build_case(case)
    want = m['state_sha256']
    state = f.state_dict()
    assert list(state) == list(want)
    for k, v in state.items():
        assert ch.sha(v) == want[k], (case, k)


@pytest.mark.parametrize('name', sorted(sh.golden().meta['nets']))
def test_equivariant_net_matches_reference_bit_for_bit(name):
    g = sh.golden()
    m = g.meta['nets'][name]
    torch.manual_seed(m['seed'])
    net = st.net.EquivariantNet(*m['args'], **m['kwargs'])
    for k, v in net.state_dict().items():
        assert ch.sha(v) == m['state_sha256'][k], (name, k)
    x, mask = g.t(f'net/{name}/x'), g.t(f'net/{name}/mask')
    with torch.no_grad():
        assert torch.equal(net(x), g.t(f'net/{name}/y'))
        assert torch.equal(net(x, mask=None), g.t(f'net/{name}/y'))
        assert torch.equal(net(x, mask), g.t(f'net/{name}/y_masked'))
        assert torch.equal(net(x, mask=mask), g.t(f'net/{name}/y_masked'))


def _closed_form_trace(net, tc, t, x, lat):
    """tr_i from the constants, the formula of set_trace_constants's docstring, in fp64 torch ops."""
    layers = list(net.net.layers)
    h = torch.cat([torch.full_like(x[..., :1], t), x] + ([] if lat is None else [lat]), -1)
    act, ds = net.net.activation, []
    for l in layers[:-1]:
        z = l(h).detach().requires_grad_(True)
        h = act(z)
        ds.append(torch.autograd.grad(h.sum(), z)[0])          # act'(z), elementwise
        h = h.detach()
    if len(ds) == 1:
        d1 = ds[0]
        return d1 @ tc[0] + d1.sum(-2, keepdim=True) @ tc[1]
    d1, d2 = ds
    s1, s2 = d1.sum(-2, keepdim=True), d2.sum(-2, keepdim=True)
    Cabd, Cc, Ce, Cf, Cg = tc
    bil = lambda p, C, q: ((p @ C) * q).sum(-1)
    return bil(d2, Cabd, d1) + bil(d2, Cc, s1) + bil(s2, Cf, d1) + (bil(d2, Ce, d1).sum(-1, keepdim=True) + bil(s2, Cg, s1))


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('hidden', [[5], [5, 6]])
@pytest.mark.parametrize('n,latent', [(1, 0), (2, 2), (5, 0), (5, 2)])
def test_set_trace_constants_against_autograd(n, latent, hidden, act):
    """fp64 rounding of O(100) terms: per-element trace error <= 1e-12 * max(1, max |tr|)."""
    torch.manual_seed(7)
    dim = 3
    net = st.net.DiffeqDeepset(1 + dim + latent, hidden, dim, activation=act).double()
    with torch.no_grad():
        for l in net.net.layers:
            l.l1.bias.normal_()
            l.l2.bias.normal_()
    x = torch.randn(2, n, dim, dtype=torch.float64)
    lat = torch.randn(2, n, latent, dtype=torch.float64) if latent else None
    t = 0.3
    tc = cnf.set_trace_constants([(l.l1.weight.detach(), l.l2.weight.detach()) for l in net.net.layers], dim, n)
    assert tc.dtype == torch.float64 and tc.shape == ((2, hidden[0]) if len(hidden) == 1 else (5, hidden[1], hidden[0]))
    got = _closed_form_trace(net, tc, t, x, lat)
    v = x.clone().requires_grad_(True)
    dv = net(torch.tensor([t], dtype=torch.float64), v, latent=lat)
    want = st.util.divergence_exact_for_sets(dv, v).sum(-1).detach()
    own = sh.set_divergence64(dv, v).detach()                   # (the batched form the fp64 restatement uses)
    assert (want - own).abs().max().item() <= 1e-14 * max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * max(1.0, want.abs().max().item()), (err, want.abs().max().item())


@pytest.mark.parametrize('case', [c for c in sh.case_names() if '/T0.7/' in c and ('/rk4/' in c or '2x7x3' in c)])
def test_composition_path_reproduces_fixture_bit_for_bit(case):
    g = sh.golden()
    f, x, lat, m = sh.build_case(case)
    y, l = f._composed_reference(x, lat)
    assert torch.equal(y, g.t(f'{case}/y')) and torch.equal(l, g.t(f'{case}/ldj'))
    xb, lb = f._composed_reference(g.t(f'{case}/y'), lat, reverse=True)
    assert torch.equal(xb, g.t(f'{case}/x_back')) and torch.equal(lb, g.t(f'{case}/ldj_back'))
    assert l.shape == (*m['shape'][:-1], 1)


def test_restatement_agrees_with_fixture():
    """The fp64 restatement (sethelp.solve64) sits within fp32 rounding of the reference's fp32 solve, masks included in its net."""
    g = sh.golden()
    for case in [c for c in sh.case_names() if '/rk4/T0.7/l3' in c]:
        f, x, lat, _ = sh.build_case(case)
        y64, l64 = sh.solve64(f, x, lat)
        assert (g.t(f'{case}/y').double() - y64).abs().max().item() <= 1e-5
        assert (g.t(f'{case}/ldj').double() - l64).abs().max().item() <= 1e-5
    name = 'tanh'
    m = g.meta['nets'][name]
    torch.manual_seed(m['seed'])
    net = st.net.DiffeqDeepset(*m['args'], **m['kwargs'])
    f = st.ContinuousTransform(3, net=net, solver='euler')
    x, mask = g.t(f'net/{name}/x'), g.t(f'net/{name}/mask')
    got = sh.deepset64(f)(0.0, x[..., 1:].double(), None, mask.double())
    want = net.net(torch.cat([torch.zeros_like(x[..., :1]), x[..., 1:]], -1), mask).detach()
    assert (got - want.double()).abs().max().item() <= 1e-6


def _desc(dim, hidden, latent=0, n=4, act=1):
    d = _hip.sx_cnf_set_net()
    d.n_layers, d.dim, d.latent_dim, d.act, d.set_size = len(hidden) + 1, dim, latent, act, n
    for i, w in enumerate((list(hidden) + [dim])[:3]):
        d.out_dim[i] = w
    return d


def test_lds_bytes_coverage_gate():
    lib = _hip.lib()
    for dim, hidden, latent, n in ((2, [64, 64], 0, 32), (32, [64, 64], 31, 128), (1, [1], 0, 1), (3, [16], 3, 7), (32, [64], 0, 128),
                                   (5, [33, 20], 0, 2)):
        for want in (0, 1):
            b = lib.sx_cnf_set_lds_bytes(_desc(dim, hidden, latent, n), want)
            assert 0 < b <= _hip.CNF_LDS_BYTES, (dim, hidden, latent, n, want, b)
    for d in (_desc(2, [65]), _desc(2, [64, 65]), _desc(33, [16]), _desc(2, [8, 8, 8]), _desc(2, [16], n=129), _desc(2, [16], n=0),
              _desc(2, [16], latent=62), _desc(2, [16], act=7)):
        assert lib.sx_cnf_set_lds_bytes(d, 1) == 0
    d = _desc(2, [16])
    d.out_dim[1] = 3
    assert lib.sx_cnf_set_lds_bytes(d, 1) == 0                  # the last layer must map back to dim
    assert lib.sx_cnf_set_lds_bytes(None, 1) == 0


def test_kernel_plan_gate_and_constants_cache():
    """`_set_kernel_net` (host only: it reads shapes and builds the constants): what is offered to the kernel and what is not; the
    constants are cached per set size and rebuilt when a weight changes."""
    dev = torch.device('cpu')
    f = sh.make(2, [16, 12], latent=3)
    plan = f._set_kernel_net(5, 3, dev)
    assert plan is not None and plan[0].set_size == 5 and plan[0].n_layers == 3 and list(plan[0].out_dim) == [16, 12, 2]
    image, off = f._set_constants(list(f.odefunc.diffeq.net.layers), 5, dev)
    assert f._set_constants(list(f.odefunc.diffeq.net.layers), 5, dev)[0] is image
    assert f._set_constants(list(f.odefunc.diffeq.net.layers), 6, dev)[0] is not image
    l0 = f.odefunc.diffeq.net.layers[0]
    G0 = image[off['G0']:off['G0'] + l0.l2.weight.numel()].reshape(l0.l2.weight.shape)
    torch.testing.assert_close(G0, l0.l2.weight.detach() / 5, rtol=2e-7, atol=0)
    b0 = image[off['b0']:off['b0'] + 16]
    torch.testing.assert_close(b0, (l0.l1.bias + l0.l2.bias / 5).detach(), rtol=1e-6, atol=1e-7)
    assert all(o % 4 == 0 for o in off.values()) and image.numel() == off['trace'] + 5 * 32 * 32
    with torch.no_grad():
        l0.l2.weight.mul_(2.0)
    image2, _ = f._set_constants(list(f.odefunc.diffeq.net.layers), 5, dev)
    assert image2 is not image
    for bad in (f._set_kernel_net(129, 3, dev), f._set_kernel_net(5, 2, dev), sh.make(2, [65])._set_kernel_net(4, 0, dev),
                sh.make(33, [8])._set_kernel_net(4, 0, dev), sh.make(2, [8, 8, 8])._set_kernel_net(4, 0, dev),
                sh.make(2, [8], final_activation='Tanh')._set_kernel_net(4, 0, dev), sh.make(2, [8], activation='GELU')._set_kernel_net(4, 0, dev),
                st.ContinuousTransform(2, net=st.net.DiffeqMLP(3, [8], 2), set_data=True)._set_kernel_net(4, 0, dev)):
        assert bad is None
    g = sh.make(2, [8])
    g.odefunc.diffeq.net.activation = torch.nn.LeakyReLU(0.2)
    assert g._set_kernel_net(4, 0, dev) is None
    # the settings that take the set kernel's branch (cnf.py:91-93)
    for div, set_data, train, want in (('compute', True, False, True), ('compute', True, True, True), ('approximate', True, False, True),
                                       ('approximate', True, True, False), ('compute_set', False, True, True), ('compute', False, False, False),
                                       ('approximate', False, False, False), ('exact', True, False, False)):
        h = sh.make(2, [8], divergence=div, set_data=set_data)
        h.train(train)
        assert h.odefunc.exact_set_trace() is want, (div, set_data, train)
