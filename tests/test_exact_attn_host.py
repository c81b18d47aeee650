"""CPU: the exact-trace attention nets (DiffeqZeroTraceAttention, DiffeqExactTraceAttention) against fixture F22 -- constructor surface,
key lists, init draws, state loading --, closed_form_attn against the fixture, against autograd in fp64 and in its structure (hollow
exclusive net, equivariance, independence of batch neighbours, N = 1), the kernel's LDS image, the coverage gates, the dispatch rows and
the host-side sanitizer driver of sx_cnf_exact_attn_flow.

The nets' plain forward runs on the HIP attention core, so on the CPU the arithmetic is checked through closed_form_attn.  The fixture
is the reference's fp32 output: closed_form_attn in fp64 is held to it within cnfhelp.bound -- 8 x the error of the same closed form in
fp32 against fp64, floored at 1e-6 max(1, |fp64|) -- the series' rule for two fp32 sequences of one arithmetic.  Against autograd, fp64
against fp64, the tolerance is test_exact_set_host.py's 1e-12 max(1, |want|)."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.net import diffeq_exact_trace as xt
from stribor_amd.net import diffeq_zero_trace as zt

import cnfhelp as ch
import exactattnhelp as xh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T64 = torch.tensor([0.3], dtype=torch.float64)


def _signature(fn):
    return {k: (None if p.default is inspect.Parameter.empty else repr(p.default)) for k, p in inspect.signature(fn).parameters.items()
            if k != 'self'}


def test_constructor_surface_and_keys():
    meta = xh.golden().meta
    assert _signature(zt.DiffeqZeroTraceAttention.__init__) == meta['signatures']['DiffeqZeroTraceAttention']
    assert _signature(xt.DiffeqExactTraceAttention.__init__) == meta['signatures']['DiffeqExactTraceAttention']
    assert list(zt.DiffeqZeroTraceAttention(2, [4, 6], 6, 2).state_dict()) == meta['zero_trace_keys']
    assert list(xt.DiffeqExactTraceAttention(2, [4, 6], 2, 3, latent_dim=1, n_heads=2).state_dict()) == meta['exact_trace_keys']
    assert 'exclusive_net.q.net.0.mask' in meta['exact_trace_keys'] and 'exclusive_net.proj.net.0.weight' in meta['exact_trace_keys']
    # the two classes live in their modules; the package namespace stribor_amd.net does not re-export them (test_exact_set_host.py and
    # test_attention_cnf_host.py pin that namespace)
    net = xt.DiffeqExactTraceAttention(2, [4, 6], 2, 3)
    assert issubclass(xt.DiffeqExactTraceAttention, st.net.DiffeqExactTrace) and type(net.exclusive_net) is zt.DiffeqZeroTraceAttention
    assert st.ContinuousTransform(2, net=net, divergence='exact').set_data


def _bare(name):
    g = xh.golden()
    m = g.meta['bare'][name]
    torch.manual_seed(m['seed'])
    net = getattr(xt if m['kind'].startswith('DiffeqExact') else zt, m['kind'])(*m['args'], **m['kwargs'])
    assert list(net.state_dict()) == m['keys']
    for k, want in m['state_sha256'].items():                        # the init draw stream: q, k, v, proj, dimwise net
        assert ch.sha(net.state_dict()[k]) == want, (name, k)
    net.load_state_dict(g.state(f'bare/{name}'), strict=True)
    lat = g.t(f'bare/{name}/latent') if g.has(f'bare/{name}/latent') else None
    return net, g.t(f'bare/{name}/x'), lat, g


@pytest.mark.parametrize('name', sorted(xh.golden().meta['bare']))
def test_bare_nets_against_the_closed_form(name):
    net, x, lat, g = _bare(name)
    if name.startswith('exact'):
        f64, j64 = xt.closed_form_attn(net, 0.3, x, lat, dtype=torch.float64)
        f32, j32 = xt.closed_form_attn(net, 0.3, x, lat)
        for what, ref32, truth in (('y', f32, f64), ('jac', j32, j64)):
            tol, e_ref = ch.bound(ref32, truth)
            err = (g.t(f'bare/{name}/{what}').double() - truth).abs().max().item()
            print(f'{name} {what}: fixture - fp64 {err:.3e}, fp32 closed form - fp64 {e_ref:.3e}, bound {tol:.3e}')
            assert err <= tol, (name, what)
        assert xt.closed_form_attn(net, 0.3, x, lat, want_jac=False)[1] is None
    else:
        # the exclusive net alone: h of the closed form, dimension-major [..., N, D * k]
        D, hidden, out = g.meta['bare'][name]['args']
        wrap = xt.DiffeqExactTraceAttention(D, hidden, D, out // D, n_heads=g.meta['bare'][name]['kwargs'].get('n_heads', 1))
        wrap.exclusive_net = net
        s = xt._structure_attn(wrap)
        want = g.t(f'bare/{name}/y')
        h64 = xt._attn_exclusive(s, x.double(), torch.float64).reshape(want.shape)
        h32 = xt._attn_exclusive(s, x, torch.float32).reshape(want.shape)
        tol, e_ref = ch.bound(h32, h64)
        assert (want.double() - h64).abs().max().item() <= tol, name
        if g.has(f'bare/{name}/jac'):
            assert torch.all(g.t(f'bare/{name}/jac') == 0)
        if x.shape[-2] == 1:                                          # N = 1: no keys, h = the projection's bias
            assert torch.equal(h32, net.proj.net[0].bias.detach().repeat(x.shape[-1]).expand(want.shape))


def test_mask_is_declined_with_a_message():
    net = zt.DiffeqZeroTraceAttention(2, [8], 4)
    with pytest.raises(NotImplementedError, match='mask=None is the only supported call'):
        net(T64, torch.randn(3, 2), mask=torch.ones(3, 1))


@pytest.mark.parametrize('case', xh.case_names())
def test_closed_form_solve_reproduces_f22(case):
    """(also: the init draws of every case -- build_case asserts the hashes)"""
    g = xh.golden()
    f, x, lat, m = xh.build_case(case)
    assert f.set_data
    y64, l64 = xh.solve64(f, x, lat)
    y32, l32 = xh.solve32(f, x, lat)
    yb = g.t(f'{case}/y')
    xb64, lb64 = xh.solve64(f, yb, lat, reverse=True)
    xb32, lb32 = xh.solve32(f, yb, lat, reverse=True)
    for name, ref32, truth in (('y', y32, y64), ('ldj', l32, l64), ('x_back', xb32, xb64), ('ldj_back', lb32, lb64)):
        tol, _ = ch.bound(ref32, truth)
        got = g.t(f'{case}/{name}')
        assert got.shape == truth.shape
        assert (got.double() - truth).abs().max().item() <= tol, (case, name, (got.double() - truth).abs().max().item(), tol)
    assert l64.shape == (*x.shape[:-1], 1)


ACTS = ['Identity', 'Tanh', 'ReLU', 'Sigmoid', 'ELU', 'Softplus', 'LeakyReLU']


def _net64(D, hidden, d_h, latent, heads, act='Tanh', seed=0):
    torch.manual_seed(seed)
    net = xt.DiffeqExactTraceAttention(D, hidden, D, d_h, latent_dim=latent, n_heads=heads)
    xh.set_activation(net, act)
    net = net.double()
    # default-init weights, every bias non-zero (see test_exact_set_host.py on Softplus's derivative from its output)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith('bias'):
                p.normal_(0, 0.3)
    return net


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('hidden,heads', [([8], 2), ([7, 12], 4)])
def test_closed_form_attn_matches_autograd_of_its_value(act, hidden, heads):
    D = 3
    for n in (1, 2, 5):
        for latent in (0, 2):
            net = _net64(D, hidden, 3, latent, heads, act, seed=10 * n + latent)
            s = xt._structure_attn(net)
            x = torch.randn(2, n, D, dtype=torch.float64)
            lat = torch.randn(2, n, latent, dtype=torch.float64) if latent else None
            fn = lambda v: xt._attn_value(s, 0.3, v, lat, False, torch.float64)[0]
            J = torch.autograd.functional.jacobian(fn, x).reshape(2 * n * D, 2 * n * D)
            f, jac = xt.closed_form_attn(net, 0.3, x, lat)
            for what, got, want in (('f', f, fn(x)), ('jac', jac, J.diagonal().reshape(2, n, D))):
                tol = 1e-12 * max(1.0, want.abs().max().item())
                assert (got - want).abs().max().item() <= tol, (act, hidden, n, latent, what)
    x2 = torch.randn(4, D, dtype=torch.float64)                       # a 2-D input is one set
    assert torch.equal(xt.closed_form_attn(net, 0.3, x2, None if lat is None else lat[0, :1].expand(4, -1))[0],
                       xt.closed_form_attn(net, 0.3, x2[None], None if lat is None else lat[:1, :1].expand(1, 4, -1))[0][0])


@pytest.mark.parametrize('hidden,heads', [([8], 1), ([6, 8], 2)])
@pytest.mark.parametrize('n', [1, 2, 5])
def test_exclusive_net_block_diagonal_is_exactly_zero(hidden, heads, n):
    D, d_h = 3, 2
    s = xt._structure_attn(_net64(D, hidden, d_h, 0, heads, seed=n))
    x = torch.randn(2, n, D, dtype=torch.float64)
    J = torch.autograd.functional.jacobian(lambda v: xt._attn_exclusive(s, v, torch.float64).reshape(2, n, D, d_h), x)   # [2, n, D, d_h, 2, n, D]
    assert J.abs().max().item() > 0 or n == 1
    for b in range(2):
        for i in range(n):
            for d in range(D):
                assert torch.all(J[b, i, d, :, b, i, d] == 0), (b, i, d)
    if n == 1:                                                        # no keys: h is the projection's bias, whatever x
        h = xt._attn_exclusive(s, x, torch.float64)
        assert torch.equal(h, s['proj'].bias.detach().expand(2 * n, D, d_h))


def test_permutation_equivariance_and_batch_independence():
    D = 3
    net = _net64(D, [10, 8], 3, 2, 2, seed=4)
    x, lat = torch.randn(3, 6, D, dtype=torch.float64), torch.randn(3, 6, 2, dtype=torch.float64)
    f, jac = xt.closed_form_attn(net, 0.3, x, lat)
    perm = torch.randperm(6)
    fp, jp = xt.closed_form_attn(net, 0.3, x[:, perm], lat[:, perm])
    tol = 1e-13 * max(1.0, f.abs().max().item(), jac.abs().max().item())
    assert (fp - f[:, perm]).abs().max().item() <= tol and (jp - jac[:, perm]).abs().max().item() <= tol
    for b in range(3):                                                # a set alone = the set among its neighbours
        fb, jb = xt.closed_form_attn(net, 0.3, x[b:b + 1], lat[b:b + 1])
        assert (fb[0] - f[b]).abs().max().item() <= tol and (jb[0] - jac[b]).abs().max().item() <= tol
    # twins: equal x and latent -> equal outputs
    x[:, 3], lat[:, 3] = x[:, 1], lat[:, 1]
    f, jac = xt.closed_form_attn(net, 0.3, x, lat)
    assert (f[:, 3] - f[:, 1]).abs().max().item() <= tol and (jac[:, 3] - jac[:, 1]).abs().max().item() <= tol


# ---- the kernel's image -----------------------------------------------------------------------------------------------------------
def _desc(dim=3, d_h=3, latent=0, hidden=(16, 8), set_size=4, act=1, heads=2):
    d = _hip.sx_cnf_exact_attn_net()
    d.dim, d.d_h, d.latent_dim, d.n_hidden, d.act, d.set_size, d.n_heads = dim, d_h, latent, len(hidden), act, set_size, heads
    for i, w in enumerate(hidden[:2]):
        d.hidden[i] = w
    return d


# (hidden tiles, hidden layers, output tiles) -> a shape that selects the instantiation
INSTANCES = {(1, 1, 1): ([16], 2), (1, 1, 2): ([16], 3), (1, 1, 4): ([32], 8), (1, 2, 1): ([20, 8], 1), (1, 2, 2): ([32, 16], 4),
             (1, 2, 4): ([12, 8], 5), (2, 2, 1): ([33, 8], 2), (2, 2, 2): ([64, 32], 3), (2, 2, 4): ([40, 16], 8)}


@pytest.mark.parametrize('inst', sorted(INSTANCES))
def test_kernel_image_attn_size_and_masked_weights(inst):
    hidden, d_h = INSTANCES[inst]
    for D, latent in ((2, 0), (4, 35)) + (((8, 3),) if hidden[-1] <= 16 else ()):
        torch.manual_seed(5)
        net = xt.DiffeqExactTraceAttention(D, hidden, D, d_h, latent_dim=latent, n_heads=4)
        s = xt.kernel_coverage_attn(net, D, latent, 7)
        assert s is not None and s['E'] == hidden[-1] and s['heads'] == 4
        image, w_latent = xt.kernel_image_attn(s)
        im = xt._Image(s)
        assert (im.HT, im.NH, im.OT) == inst
        lds = _hip.lib().sx_cnf_exact_attn_lds_bytes(_desc(D, d_h, latent, hidden, 7, heads=4))
        assert lds == 4 * (image.size + xt.ATTN_EXCHANGE_FLOATS) and lds <= _hip.CNF_LDS_BYTES
        assert image.dtype == np.float32 and image.size % 4 == 0 and np.isfinite(image).all()
        assert (w_latent is None) == (latent == 0) and (latent == 0 or w_latent.shape == (32 * im.HT, 32 * ((latent + 31) // 32)))
        # a weight under a zero mask never reaches the image
        q = net.exclusive_net.q.masked_linears()
        assert any((l.mask == 0).any() for l in q)
        with torch.no_grad():
            for l in q:
                l.weight[l.mask == 0] = float('inf')
        again = xt.kernel_image_attn(xt.kernel_coverage_attn(net, D, latent, 7))[0]
        assert np.isfinite(again).all() and np.array_equal(again, image)
        assert len(xt.kernel_tensors_attn(s)) == 3 * len(q) + 2 * (2 * len(s['k']) + 1 + len(s['dimwise']))


def test_kernel_image_attn_query_positions():
    """The q MADE's last layer, read back: column e * D + d sits at position (d % per) * slot + e of tile d // per."""
    torch.manual_seed(2)
    D, E = 5, 12                                                      # slot 16: two dimensions a tile, three tiles
    net = xt.DiffeqExactTraceAttention(D, [E], D, 2)
    s = xt.kernel_coverage_attn(net, D, 0, 3)
    image, _ = xt.kernel_image_attn(s)
    l = s['q'][0]
    W = (l.mask * l.weight).detach().numpy()
    assert xt.attn_query_tiles(E, D) == 3
    for d in range(D):
        for e in range(E):
            row = 32 * (d // 2) + (d % 2) * 16 + e
            for i in range(D):
                col = xt._kmap(i, 0)
                r = [r for r in range(16) if xt._kmap(r, 0) == col][0]
                at = (row // 32) * 1024 + (r >> 2) * 256 + (row % 32) * 4 + (r & 3)
                assert image[at] == W[e * D + d, i], (d, e, i)
            assert image[3 * 1024 + row] == l.bias[e * D + d].item()


def test_lds_bytes_at_the_coverage_edges():
    lds = _hip.lib().sx_cnf_exact_attn_lds_bytes
    inside = [dict(), dict(dim=8), dict(d_h=8), dict(latent=64), dict(hidden=(64, 32), dim=4), dict(set_size=128), dict(set_size=1), dict(act=6),
              dict(heads=1), dict(heads=4), dict(hidden=(32,), dim=4, heads=4), dict(hidden=(64, 32), dim=2, d_h=8, set_size=128),
              dict(hidden=(32, 16), dim=8, d_h=8, set_size=128), dict(hidden=(64, 16), dim=8, d_h=8, latent=64, set_size=128)]
    outside = [dict(dim=9), dict(dim=0), dict(d_h=9), dict(d_h=0), dict(latent=65), dict(hidden=(65, 8)), dict(hidden=(16, 33)), dict(hidden=(33,)),
               dict(hidden=(0,)), dict(set_size=129), dict(set_size=0), dict(act=7), dict(heads=3), dict(heads=8), dict(heads=0),
               dict(hidden=(16, 6), heads=4), dict(hidden=(16, 17), dim=8, heads=1), dict(hidden=(16, 32), dim=5)]
    for kw in inside:
        assert 0 < lds(_desc(**kw)) <= _hip.CNF_LDS_BYTES, kw
    for kw in outside:
        assert lds(_desc(**kw)) == 0, kw
    d = _desc()
    d.n_hidden = 3
    assert lds(d) == 0
    d.n_hidden = 0
    assert lds(d) == 0
    # the two mandated shapes and the largest image, plus the exchange
    assert lds(_desc(hidden=(64, 32), dim=2, d_h=8, set_size=128)) == 4 * (22208 + xt.ATTN_EXCHANGE_FLOATS)
    assert lds(_desc(hidden=(32, 16), dim=8, d_h=8, set_size=128)) == 4 * (12800 + xt.ATTN_EXCHANGE_FLOATS)
    assert lds(_desc(hidden=(64, 16), dim=8, d_h=8, set_size=128)) == 4 * (26368 + xt.ATTN_EXCHANGE_FLOATS) == 142848


def test_library_exports_and_abi():
    lib = _hip.lib()
    assert 'sx_cnf_exact_attn_lds_bytes' in _hip.EXPORTS and 'sx_cnf_exact_attn_flow' in _hip.EXPORTS
    assert lib.sx_cnf_exact_attn_flow is not None and lib.sx_cnf_exact_attn_lds_bytes is not None
    assert lib.sx_abi_version() == 3


def test_kernel_coverage_attn_gates():
    """One step outside each bound declines."""
    mk = lambda dim=3, **kw: xt.DiffeqExactTraceAttention(dim, kw.pop('hidden', [16, 8]), dim, kw.pop('d_h', 2), **kw)
    cov = lambda net, dim=3, latent=0, n=5: xt.kernel_coverage_attn(net, dim, latent, n)
    assert cov(mk()) is not None and cov(mk(), n=128) is not None and cov(mk(), n=1) is not None
    assert cov(mk(hidden=[64, 32], n_heads=4)) is not None and cov(mk(8, hidden=[32, 16]), 8) is not None
    assert cov(mk(hidden=[33])) is None and cov(mk(hidden=[16, 33])) is None                  # E = 33
    assert cov(mk(hidden=[65, 8])) is None                                                      # H1 = 65
    assert cov(mk(9, hidden=[8]), 9) is None                                                    # dim = 9
    assert cov(mk(8, hidden=[16]), 8) is not None and cov(mk(8, hidden=[17]), 8) is None        # E * dim = 128 | 136: five tiles and more
    assert cov(mk(4, hidden=[32]), 4) is not None and cov(mk(5, hidden=[32]), 5) is None        # E * dim = 128 | 160
    assert cov(mk(hidden=[12], n_heads=3)) is None and cov(mk(hidden=[16], n_heads=8)) is None  # 3 heads, 8 heads
    assert cov(mk(d_h=9)) is None and cov(mk(d_h=8)) is not None                                # d_h = 9
    assert cov(mk(), n=129) is None                                                             # N = 129
    assert cov(mk(hidden=[8, 8, 8])) is None                                                    # three hidden dims
    assert cov(mk(latent_dim=2)) is None and cov(mk(latent_dim=65), latent=65) is None and cov(mk(latent_dim=64), latent=64) is not None
    assert cov(xh.set_activation(mk(), 'ELU', lambda: nn.ELU(alpha=2.0))) is None               # ELU(alpha=2)
    assert cov(xh.set_activation(mk(), 'ELU')) is not None

    class Sub(xt.DiffeqExactTraceAttention):
        pass
    assert cov(Sub(3, [16, 8], 3, 2)) is None                                                   # a subclass of the net
    net = mk()
    assert cov(st.net.DiffeqExactTrace(net.exclusive_net, net.dimwise_net)) is None
    net.dimwise_net.net.net[1] = nn.ReLU()                                                      # two activations in one net
    assert cov(net) is None
    assert cov(mk(return_log_det_jac=False)) is None


# ---- dispatch: rows in the style of test_cnf_dispatch_host.py ---------------------------------------------------------------------
DIM = 3
NETS = {
    'exact_attn': lambda L: xt.DiffeqExactTraceAttention(DIM, [16, 8], DIM, 2, latent_dim=L, n_heads=2),
    'exact_attn_8heads': lambda L: xt.DiffeqExactTraceAttention(DIM, [16], DIM, 2, n_heads=8),
    'exact_attn_e33': lambda L: xt.DiffeqExactTraceAttention(DIM, [33], DIM, 2),
    'exact_attn_dh9': lambda L: xt.DiffeqExactTraceAttention(DIM, [16], DIM, 9),
}
# (net, latent, divergence, set_data, training, x.shape, mask, graph wanted) -> the route
ROWS = [
    ('exact_attn', 0, 'exact', False, False, (2, 4, 3), False, False, 'sx_cnf_exact_attn_flow'),
    ('exact_attn', 0, 'exact', True, False, (2, 4, 3), False, False, 'sx_cnf_exact_attn_flow'),
    ('exact_attn', 2, 'exact', True, True, (2, 2, 4, 3), False, False, 'sx_cnf_exact_attn_flow'),
    ('exact_attn', 0, 'exact', False, False, (5, 3), False, False, 'sx_cnf_exact_attn_flow'),          # a 2-D x is one set
    ('exact_attn', 0, 'exact', True, False, (1, 3), False, False, 'sx_cnf_exact_attn_flow'),
    ('exact_attn', 0, 'exact', False, False, (2, 128, 3), False, False, 'sx_cnf_exact_attn_flow'),
    ('exact_attn', 0, 'exact', False, False, (2, 4, 3), True, False, 'composed'),
    ('exact_attn', 0, 'exact', False, False, (2, 4, 3), False, True, 'composed'),
    ('exact_attn', 0, 'none', False, False, (2, 4, 3), False, False, 'composed'),
    ('exact_attn', 0, 'none', True, False, (2, 4, 3), False, False, 'composed'),
    ('exact_attn', 0, 'exact', False, False, (2, 129, 3), False, False, 'composed'),
    ('exact_attn_8heads', 0, 'exact', False, False, (2, 4, 3), False, False, 'composed'),
    ('exact_attn_e33', 0, 'exact', False, False, (2, 4, 3), False, False, 'composed'),
    ('exact_attn_dh9', 0, 'exact', True, False, (2, 4, 3), False, False, 'composed'),
]
_made = {}


@pytest.mark.parametrize('row', ROWS, ids=lambda r: '-'.join(str(v) for v in r[:8]))
def test_route(row):
    net, latent, divergence, set_data, training, shape, masked, graph, want = row
    key = (net, latent, divergence, set_data)
    if key not in _made:
        _made[key] = st.ContinuousTransform(DIM, net=NETS[net](latent), divergence=divergence, has_latent=latent > 0, solver='rk4',
                                            solver_options={'step_size': 0.25}, set_data=set_data)
    f = _made[key].train(training)
    for want_ldj in (True, False):
        route, plan, trace = f._choose(torch.Size(shape), latent, masked, graph, want_ldj, torch.device('cpu'))
        assert route == want
        assert (plan is None) == (route == 'composed')
        assert trace == (want_ldj and divergence != 'none')
        if plan is not None:
            assert type(plan[0]) is _hip.sx_cnf_exact_attn_net and plan[0].set_size == shape[-2] and plan[0].n_heads == 2


def test_plan_cache_follows_weights_and_masks():
    """The image is cached under guards on weights, biases AND masks: an in-place edit of either rebuilds it."""
    f = xh.make(3, [16, 8], 2, heads=2)
    plan = lambda: f._choose(torch.Size((2, 4, 3)), 0, False, False, True, torch.device('cpu'))[1]
    a = plan()[1][0]
    assert plan()[1][0] is a
    q = f.odefunc.diffeq.exclusive_net.q.masked_linears()
    with torch.no_grad():
        q[0].weight.mul_(1.5)
    b = plan()[1][0]
    assert b is not a and not torch.equal(a, b)
    i, j = [int(v[0]) for v in torch.nonzero(q[-1].mask, as_tuple=True)]
    with torch.no_grad():
        q[-1].mask[i, j] = 0
    c = plan()[1][0]
    assert c is not b and not torch.equal(b, c)


def test_host_code_under_sanitizers():
    """`make asan_exact_attn`: the library's host code (--offload-host-only, -fsanitize=address,undefined) linked with
    tests/asan_exact_attn_driver.cpp, a stand-alone program that drives sx_cnf_exact_attn_lds_bytes / sx_cnf_exact_attn_flow's validators
    without a GPU.  No sanitizer report, no accepted bad call."""
    csrc = os.path.join(ROOT, 'stribor_amd', 'csrc')
    b = subprocess.run(['make', '-C', csrc, '-j', str(min(8, os.cpu_count() or 1)), 'asan_exact_attn'], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(csrc, 'asan', 'asan_exact_attn_driver')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    assert ' 0 failures' in r.stdout, r.stdout[-1500:]
