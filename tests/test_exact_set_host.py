"""CPU: the exact-trace set nets (DiffeqZeroTraceDeepSet, DiffeqExactTraceDeepSet) against fixture F19 -- constructor surface, key
lists, init draws, bare nets and the composed solve bit for bit --, the hollow block Jacobian, closed_form_set against autograd in
fp64, the kernel's LDS image read back position by position, and the coverage edges of sx_cnf_exact_set_lds_bytes."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn as nn

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.net import diffeq_exact_trace as xt
from stribor_amd.net import diffeq_zero_trace as zt

import cnfhelp as ch
import exactsethelp as xh

T03 = torch.tensor([0.3])
T64 = torch.tensor([0.3], dtype=torch.float64)


def _signature(fn):
    return {k: (None if p.default is inspect.Parameter.empty else repr(p.default)) for k, p in inspect.signature(fn).parameters.items()
            if k != 'self'}


def test_constructor_surface_and_keys():
    meta = xh.golden().meta
    assert _signature(st.net.DiffeqZeroTraceDeepSet.__init__) == meta['signatures']['DiffeqZeroTraceDeepSet']
    assert _signature(st.net.DiffeqExactTraceDeepSet.__init__) == meta['signatures']['DiffeqExactTraceDeepSet']
    assert _signature(zt.ZeroTraceEquivariantEncoder.__init__) == meta['encoder_signature']
    assert list(st.net.DiffeqZeroTraceDeepSet(2, [4, 5], 6).state_dict()) == meta['zero_trace_keys']
    assert list(st.net.DiffeqExactTraceDeepSet(2, [4, 5], 2, 3, latent_dim=1).state_dict()) == meta['exact_trace_keys']
    assert not hasattr(st.net, 'DiffeqExactTraceAttention') and not hasattr(st.net, 'DiffeqZeroTraceAttention')


def _bare(name):
    g = xh.golden()
    m = g.meta['bare'][name]
    torch.manual_seed(m['seed'])
    net = getattr(st.net, m['kind'])(*m['args'], **m['kwargs'])
    assert list(net.state_dict()) == m['keys']
    for k, want in m['state_sha256'].items():                        # the init draw stream: MADE, set embedding, dimwise net
        assert ch.sha(net.state_dict()[k]) == want, (name, k)
    net.load_state_dict(g.state(f'bare/{name}'), strict=True)
    lat = g.t(f'bare/{name}/latent') if g.has(f'bare/{name}/latent') else None
    return net, g.t(f'bare/{name}/x'), lat, g


@pytest.mark.parametrize('name', sorted(xh.golden().meta['bare']))
def test_bare_nets_bit_for_bit(name):
    net, x, lat, g = _bare(name)
    out = net(T03, x, latent=lat) if name.startswith('exact') else net(T03, x)          # (with a graph: plain torch on the CPU)
    out = tuple(o.detach() for o in out) if isinstance(out, tuple) else out.detach()
    if isinstance(out, tuple):
        assert torch.equal(out[0], g.t(f'bare/{name}/y')) and torch.equal(out[1], g.t(f'bare/{name}/jac'))
    else:
        assert not g.has(f'bare/{name}/jac') and torch.equal(out, g.t(f'bare/{name}/y'))


def test_init_draws_of_every_case():
    for case in xh.case_names():
        xh.build_case(case)                                           # (asserts the hashes)


@pytest.mark.parametrize('pooling', ['max', 'mean', 'sum'])
@pytest.mark.parametrize('n', [1, 2, 5])
def test_zero_trace_block_jacobian_is_hollow(pooling, n):
    torch.manual_seed(n)
    D, k = 3, 2
    net = st.net.DiffeqZeroTraceDeepSet(D, [7, 6], k * D, pooling=pooling, return_log_det_jac=False).double()
    x = torch.randn(2, n, D, dtype=torch.float64)
    J = torch.autograd.functional.jacobian(lambda v: net(T64, v), x)          # [2, n, D k, 2, n, D]
    assert J.abs().max().item() > 0 or n == 1
    for b in range(2):
        for i in range(n):
            for d in range(D):
                assert torch.all(J[b, i, d * k:(d + 1) * k, b, i, d] == 0), (b, i, d)
    y, div = st.net.DiffeqZeroTraceDeepSet(D, [7], k * D, pooling=pooling)(T03, x.float())
    assert y.shape == (2, n, D * k) and div.shape == x.shape and torch.all(div == 0)


ACTS = ['Identity', 'Tanh', 'ReLU', 'Sigmoid', 'ELU', 'Softplus', 'LeakyReLU']


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('hidden', [[9], [7, 10]])
def test_closed_form_set_matches_autograd(act, hidden):
    for n in (1, 2, 5):
        for latent in (0, 2):
            for pooling in ('max', 'mean', 'sum'):
                torch.manual_seed(10 * n + latent)
                D = 3
                net = st.net.DiffeqExactTraceDeepSet(D, hidden, D, 3, latent_dim=latent, pooling=pooling)
                xh.set_activation(net, act)
                net = net.double()
                # default-init weights, every bias non-zero: act' is taken from the activation's OUTPUT, and Softplus's 1 - exp(-a)
                # rounds to eps / a -- pre-activations of O(1) keep a >= 1e-3, i.e. that error below 1e-13
                with torch.no_grad():
                    for k, p in net.named_parameters():
                        if k.endswith('bias'):
                            p.normal_(0, 0.3)
                x = torch.randn(2, n, D, dtype=torch.float64)
                lat = torch.randn(2, n, latent, dtype=torch.float64) if latent else None
                fn = lambda v: net(T64, v, latent=lat)[0]
                J = torch.autograd.functional.jacobian(fn, x).reshape(2 * n * D, 2 * n * D)
                f, jac = xt.closed_form_set(net, 0.3, x, lat)
                f0, jac0 = net(T64, x, latent=lat)
                for what, got, want in (('f', f, fn(x)), ('jac', jac, J.diagonal().reshape(2, n, D)), ('jac0', jac0, J.diagonal().reshape(2, n, D))):
                    tol = 1e-12 * max(1.0, want.abs().max().item())
                    assert (got - want).abs().max().item() <= tol, (act, hidden, n, latent, pooling, what)
                assert xt.closed_form_set(net, 0.3, x, lat, want_jac=False)[1] is None
    x2 = torch.randn(4, D, dtype=torch.float64)                       # a 2-D input is one set
    assert torch.equal(xt.closed_form_set(net, 0.3, x2, None if lat is None else lat[0, :1].expand(4, -1))[0],
                       xt.closed_form_set(net, 0.3, x2[None], None if lat is None else lat[:1, :1].expand(1, 4, -1))[0][0])


@pytest.mark.parametrize('case', xh.case_names())
def test_composed_cpu_solve_reproduces_f19(case):
    g = xh.golden()
    f, x, lat, m = xh.build_case(case)
    y, l = f._composed_reference(x, lat)
    xb, lb = f._composed_reference(g.t(f'{case}/y'), lat, reverse=True)
    assert f.set_data
    for name, got in (('y', y), ('ldj', l), ('x_back', xb), ('ldj_back', lb)):
        assert torch.equal(got, g.t(f'{case}/{name}')), (case, name, (got - g.t(f'{case}/{name}')).abs().max().item())
    assert l.shape == (*x.shape[:-1], 1)


def _tile_value(image, base, mt_kt, m, c, row, col):
    """Entry (32m + row, 32c + col) of an image of tiles at float `base`, by the documented fragment order."""
    KT = mt_kt[1]
    for r in range(16):
        for h in range(2):
            if xt._kmap(r, h) == col:
                g, j, lane = r >> 2, r & 3, 32 * h + row
                return image[base + (m * KT + c) * 1024 + g * 256 + lane * 4 + j]
    raise AssertionError(col)


@pytest.mark.parametrize('hidden,d_h,latent', [([40], 3, 0), ([20, 33], 5, 35)])
def test_kernel_image_set_position_by_position(hidden, d_h, latent):
    torch.manual_seed(5)
    D = 5
    net = st.net.DiffeqExactTraceDeepSet(D, hidden, D, d_h, latent_dim=latent, pooling='sum')
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith('bias'):
                p.normal_()
    s = xt.kernel_coverage_set(net, D, latent, 4)
    assert s is not None and s['pooling'] == 'sum'
    image, w_latent = xt.kernel_image_set(s)
    HT, OT, NH = max(xt._tiles(w) for w in hidden), xt._out_tiles(d_h), len(hidden)
    npy = lambda p: p.detach().numpy()
    off = 0
    seen = np.zeros(image.size, bool)

    def check_mat(mt, kt, rpos, cpos, W):
        nonlocal off
        dense = np.zeros((32 * mt, 32 * kt), np.float32)
        for m in range(mt):
            for c in range(kt):
                for row in range(32):
                    for col in range(32):
                        dense[32 * m + row, 32 * c + col] = _tile_value(image, off, (mt, kt), m, c, row, col)
        want = np.zeros_like(dense)
        want[np.ix_(rpos, cpos)] = W
        assert np.array_equal(dense, want)
        seen[off:off + mt * kt * 1024] = True
        off += mt * kt * 1024

    def check_vec(nt, pos, v):
        nonlocal off
        want = np.zeros(32 * nt, np.float32)
        want[pos] = v
        assert np.array_equal(image[off:off + 32 * nt], want)
        seen[off:off + 32 * nt] = True
        off += 32 * nt

    pos_x = np.array([xt._kmap(i, 0) for i in range(D)])
    pos_raw = np.array([32 * (kk >> 1) + xt._kmap(i, kk & 1) for kk in range(d_h) for i in range(D)])
    pos_e = np.array([xt._kmap(kk >> 1, kk & 1) for kk in range(d_h)])
    pos_in = np.array([0] + [xt._kmap(1 + (kk >> 1), kk & 1) for kk in range(d_h)])
    made = net.exclusive_net.elementwise.masked_linears()
    in_pos = pos_x
    for i, l in enumerate(made):
        last = i + 1 == len(made)
        out_pos = pos_raw if last else np.arange(l.out_features)
        check_mat(OT if last else HT, 1 if i == 0 else HT, out_pos, in_pos, npy(l.mask) * npy(l.weight))
        check_vec(OT if last else HT, out_pos, npy(l.bias))
        in_pos = out_pos
    emb = [l for l in net.exclusive_net.interaction.set_emb.net.net if isinstance(l, nn.Linear)]
    in_pos = pos_x
    for i, l in enumerate(emb):
        last = i + 1 == len(emb)
        out_pos = pos_e if last else np.arange(l.out_features)
        check_mat(1 if last else HT, 1 if i == 0 else HT, out_pos, in_pos, npy(l.weight)[:, 1:] if i == 0 else npy(l.weight))
        check_vec(1 if last else HT, out_pos, npy(l.bias))
        if i == 0:
            check_vec(HT, out_pos, npy(l.weight)[:, 0])
        in_pos = out_pos
    dw = [l for l in net.dimwise_net.net.net if isinstance(l, nn.Linear)]
    W1 = npy(dw[0].weight)
    h1 = np.arange(W1.shape[0])
    check_mat(HT, 1, h1, pos_in, W1[:, 1:2 + d_h])
    check_vec(HT, h1, npy(dw[0].bias))
    check_vec(HT, h1, W1[:, 0])
    check_vec(HT, h1, W1[:, 1])
    if NH == 2:
        check_mat(HT, HT, np.arange(hidden[1]), h1, npy(dw[1].weight))
        check_vec(HT, np.arange(hidden[1]), npy(dw[1].bias))
    check_vec(HT, np.arange(hidden[-1]), npy(dw[-1].weight)[0])
    check_vec(1, np.arange(1), npy(dw[-1].bias))
    assert off == image.size and seen.all()
    if latent:
        assert w_latent.shape == (32 * HT, 64) and np.array_equal(w_latent[:hidden[0], :latent], W1[:, 2 + d_h:])
        assert not w_latent[hidden[0]:].any() and not w_latent[:, latent:].any()
    else:
        assert w_latent is None
    d = _desc(D, d_h, latent, hidden, 4)
    assert _hip.lib().sx_cnf_exact_set_lds_bytes(d) == 4 * (image.size + xt.SET_EXCHANGE_FLOATS)
    # a weight under a zero mask never reaches the image
    with torch.no_grad():
        for l in made:
            l.weight[l.mask == 0] = float('inf')
    assert np.array_equal(xt.kernel_image_set(xt.kernel_coverage_set(net, D, latent, 4))[0], image)
    assert len(xt.kernel_tensors_set(s)) == 3 * len(made) + 2 * len(emb) + 2 * len(dw)


def _desc(dim=3, d_h=3, latent=0, hidden=(16,), set_size=4, act=1, pooling=2):
    d = _hip.sx_cnf_exact_set_net()
    d.dim, d.d_h, d.latent_dim, d.n_hidden, d.act, d.set_size, d.pooling = dim, d_h, latent, len(hidden), act, set_size, pooling
    for i, w in enumerate(hidden[:2]):
        d.hidden[i] = w
    return d


def test_lds_bytes_at_the_coverage_edges():
    lds = _hip.lib().sx_cnf_exact_set_lds_bytes
    inside = [dict(), dict(dim=16), dict(d_h=8), dict(latent=64), dict(hidden=(64, 64)), dict(set_size=128), dict(set_size=1), dict(act=6),
              dict(pooling=0), dict(dim=16, d_h=8, hidden=(64, 64), latent=64, set_size=128)]
    outside = [dict(dim=17), dict(dim=0), dict(d_h=9), dict(d_h=0), dict(latent=65), dict(hidden=(65,)), dict(hidden=(64, 65)),
               dict(hidden=(0,)), dict(set_size=129), dict(set_size=0), dict(act=7), dict(pooling=3), dict(pooling=-1)]
    for kw in inside:
        assert 0 < lds(_desc(**kw)) <= _hip.CNF_LDS_BYTES, kw
    for kw in outside:
        assert lds(_desc(**kw)) == 0, kw
    d = _desc()
    d.n_hidden = 3
    assert lds(d) == 0
    d.n_hidden = 0
    assert lds(d) == 0
    # the largest image: one MADE, the embedding and the dimwise net at [64, 64], d_h = 8, plus the exchange
    assert lds(_desc(dim=16, d_h=8, hidden=(64, 64))) == 4 * (14592 + 8416 + 6496 + 2048)


def test_library_exports_and_abi():
    lib = _hip.lib()
    assert 'sx_cnf_exact_set_lds_bytes' in _hip.EXPORTS and 'sx_cnf_exact_set_flow' in _hip.EXPORTS
    assert lib.sx_cnf_exact_set_flow is not None and lib.sx_cnf_exact_set_lds_bytes is not None
    assert lib.sx_abi_version() == 3


def test_kernel_coverage_set_gates():
    mk = lambda **kw: st.net.DiffeqExactTraceDeepSet(3, kw.pop('hidden', [16]), 3, kw.pop('d_h', 2), **kw)
    assert xt.kernel_coverage_set(mk(), 3, 0, 5) is not None
    assert xt.kernel_coverage_set(mk(), 3, 0, 129) is None
    assert xt.kernel_coverage_set(mk(hidden=[65]), 3, 0, 5) is None
    assert xt.kernel_coverage_set(mk(hidden=[8, 8, 8]), 3, 0, 5) is None
    assert xt.kernel_coverage_set(mk(d_h=9), 3, 0, 5) is None
    assert xt.kernel_coverage_set(mk(latent_dim=2), 3, 0, 5) is None
    net = mk()
    assert xt.kernel_coverage_set(st.net.DiffeqExactTrace(net.exclusive_net, net.dimwise_net), 3, 0, 5) is None
    net.dimwise_net.net.net[1] = nn.ReLU()
    assert xt.kernel_coverage_set(net, 3, 0, 5) is None
    net = mk()
    net.exclusive_net.interaction.pooling = 'median'
    assert xt.kernel_coverage_set(net, 3, 0, 5) is None


def test_kernel_image_set_stages_zeros_for_a_layer_without_bias():
    """Every bias vector of the image comes from one builder branch: a layer with `bias = None` stages what a zero bias stages."""
    torch.manual_seed(6)
    D, hidden, d_h = 3, [20, 20], 3
    net = st.net.DiffeqExactTraceDeepSet(D, hidden, D, d_h, latent_dim=2, pooling='max')
    linears = [m for m in net.modules() if isinstance(m, nn.Linear)]
    assert len(linears) == 9
    with torch.no_grad():
        for l in linears:
            l.bias.normal_()
    with_bias = xt.kernel_image_set(xt.kernel_coverage_set(net, D, 2, 4))
    with torch.no_grad():
        for l in linears:
            l.bias.zero_()
    zero_bias = xt.kernel_image_set(xt.kernel_coverage_set(net, D, 2, 4))
    for l in linears:
        l.bias = None
    s = xt.kernel_coverage_set(net, D, 2, 4)
    assert s is not None and all(t is not None for t in xt.kernel_tensors_set(s))
    no_bias = xt.kernel_image_set(s)
    assert np.array_equal(no_bias[0], zero_bias[0]) and np.array_equal(no_bias[1], zero_bias[1])
    assert not np.array_equal(with_bias[0], zero_bias[0]) and np.array_equal(with_bias[1], zero_bias[1])
