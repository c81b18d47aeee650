"""GPU: EquivariantNet on sx_equivariant_fwd / sx_equivariant_bwd -- fixture F18's nets, the shape edges of the set layout and of
the two coverages, masks, set independence, determinism, input layouts, the pass loop, the gates, a set_data coupling over the net,
and the CNF paths that must not see the kernel.

Tolerances are cnfhelp.bound's: the fp32 torch module on the CPU (the fixture for the F18 cases) has its own error against a
deepcopy(net).double() on the CPU; the kernel must stay within 8 x that of the fp64 values (floor 1e-6 * max(1, max |fp64|))."""
import copy

import pytest
import torch

import stribor_amd as st
from stribor_amd.net.equivariant import EquivariantNet

import cnfhelp as ch
import passhelp as ph
import sethelp as sh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _check(tag, got, ref, truth):
    tol, e_ref = ch.bound(ref, truth)
    err = (got.detach().cpu().double() - truth).abs().max().item()
    print(f'{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e}')
    assert got.shape == truth.shape
    assert err <= tol, (tag, err, e_ref, tol)


def _params(net):
    return [p for l in net.layers for p in (l.l1.weight, l.l1.bias, l.l2.weight, l.l2.bias)]


NAMES = ['dx'] + [f'd{n}{l}' for l in range(3) for n in 'AaBb']


def _cpu(net, x, mask, gy, dtype):
    """The torch module on the CPU in `dtype`: y and, with gy, the gradients of (x, every parameter) by autograd."""
    n = copy.deepcopy(net).to(dtype)
    xx = x.detach().cpu().to(dtype).requires_grad_(gy is not None)
    y = n.forward_twice_differentiable(xx, mask=None if mask is None else mask.detach().cpu().to(dtype))
    if gy is None:
        return y.detach(), None
    return y.detach(), torch.autograd.grad(y, [xx] + _params(n), gy.cpu().to(dtype))


def _gpu(net, x, mask, gy):
    xx = x.detach().requires_grad_(True)
    y = net(xx, mask=mask)
    path = net._last_path
    return y.detach(), torch.autograd.grad(y, [xx] + _params(net), gy), path


def _full_check(tag, net, x, mask=None, graph_path='kernel', seed=0):
    """Forward (no grad: always the kernel) and a graph call with every gradient, against fp64 within the fp32 sequence's bound."""
    g = torch.Generator().manual_seed(seed)
    out = net.layers[-1].l1.out_features
    gy = torch.randn(*x.shape[:-1], out, generator=g)
    y32, g32 = _cpu(net, x, mask, gy, torch.float32)
    y64, g64 = _cpu(net, x, mask, gy, torch.float64)
    dev = copy.deepcopy(net).to(DEV)
    xd, md = x.to(DEV), None if mask is None else mask.to(DEV)
    with torch.no_grad():
        y = dev(xd, mask=md)
    assert dev._last_path == 'kernel', tag
    assert y.dtype == torch.float32
    _check(f'{tag} y', y, y32, y64)
    yg, grads, path = _gpu(dev, xd, md, gy.to(DEV))
    assert path == graph_path, (tag, path)
    _check(f'{tag} y [graph, {path}]', yg, y32, y64)
    for name, got, ref, truth in zip(NAMES, grads, g32, g64):
        _check(f'{tag} {name} [{path}]', got, ref, truth)
    return dev


def _net(seed, *args, **kw):
    torch.manual_seed(seed)
    return EquivariantNet(*args, **kw)


@pytest.mark.parametrize('name', sorted(sh.golden().meta['nets']))
def test_f18_nets(name):
    g = sh.golden()
    m = g.meta['nets'][name]
    torch.manual_seed(m['seed'])
    net = EquivariantNet(*m['args'], **m['kwargs'])
    x, mask = g.t(f'net/{name}/x'), g.t(f'net/{name}/mask')
    dev = copy.deepcopy(net).to(DEV)
    assert dev.kernel_plan(x.shape, False, torch.device(DEV)) is not None
    for tag, mk, want in (('y', None, g.t(f'net/{name}/y')), ('y_masked', mask, g.t(f'net/{name}/y_masked'))):
        y64, _ = _cpu(net, x, mk, None, torch.float64)
        with torch.no_grad():
            y = dev(x.to(DEV), mask=None if mk is None else mk.to(DEV))
        assert dev._last_path == 'kernel'
        _check(f'net/{name} {tag}', y, want, y64)


# name: ((B, N, in, hidden, out), activation, final activation, the graph call's path)
EDGES = {
    'n1_no_exchange': ((3, 1, 3, [5], 2), 'Tanh', None, 'kernel'),
    'n5_sets_straddle_waves': ((27, 5, 7, [16], 4), 'ReLU', 'Tanh', 'kernel'),
    'n5_two_hidden': ((27, 5, 7, [16, 12], 4), 'Sigmoid', None, 'kernel'),
    'n7_two_tile_output': ((6, 7, 20, [24], 40), 'ELU', 'Softplus', 'kernel'),
    'n33_padding_two_tiles_three_tile_output': ((4, 33, 33, [33, 40], 65), 'Softplus', None, 'composed'),
    'n128_widest_global_weights': ((2, 128, 64, [64, 64], 128), 'Tanh', 'Sigmoid', 'composed'),
    'bwd_edge_inside': ((2, 128, 32, [32, 32], 64), 'LeakyReLU', 'LeakyReLU', 'kernel'),
    'bwd_edge_inside_one_hidden_64': ((5, 4, 32, [64], 32), 'Tanh', None, 'kernel'),
    'bwd_edge_outside_in33': ((2, 128, 33, [32, 32], 64), 'Tanh', None, 'composed'),
    'bwd_edge_outside_hidden33': ((5, 4, 32, [33, 32], 32), 'Tanh', None, 'composed'),
    'fwd_two_tile_input': ((2, 3, 40, [8], 3), 'Tanh', None, 'composed'),
    'fwd_two_tile_input_and_hidden': ((2, 3, 40, [48], 3), 'Identity', 'ReLU', 'composed'),
    'fwd_two_tile_hidden_two_layers': ((2, 3, 5, [40, 8], 3), 'Tanh', None, 'composed'),
    'fwd_two_tile_input_two_layers': ((2, 3, 40, [8, 8], 3), 'Tanh', None, 'composed'),
}


@pytest.mark.parametrize('name', sorted(EDGES))
def test_shape_edges(name):
    (B, N, D, hidden, out), act, fact, path = EDGES[name]
    net = _net(11, D, hidden, out, activation=act, final_activation=fact)
    x = torch.randn(B, N, D, generator=ph.generator(name))
    _full_check(name, net, x, None, path)


MB, MN = 6, 7


def _mask(kind):
    g = ph.generator('mask-' + kind)
    if kind == 'binary':
        m = (torch.rand(MB, MN, 1, generator=g) < 0.5).float()
        m[:, 3] = 1.0
        return m
    if kind == 'ones':
        return torch.ones(MB, MN, 1)
    if kind == 'fractional':
        return 0.25 + torch.rand(MB, MN, 1, generator=g)
    m = (torch.rand(MB, MN, 3, generator=g) < 0.5).float()          # 'three_columns': column 0 is the mask
    m[:, 2, 0] = 1.0
    return m


@pytest.mark.parametrize('kind,act', [('binary', 'Tanh'), ('ones', 'Tanh'), ('fractional', 'Sigmoid'), ('three_columns', 'Softplus')])
def test_masks(kind, act):
    net = _net(12, 4, [12], 3, activation=act)
    x = torch.randn(MB, MN, 4, generator=ph.generator('mask-x'))
    mask = _mask(kind)
    dev = _full_check(f'mask {kind}', net, x, mask)
    if kind == 'three_columns':               # read in place: the same bits as the column on its own
        with torch.no_grad():
            md = mask.to(DEV)
            assert torch.equal(dev(x.to(DEV), mask=md), dev(x.to(DEV), mask=md[..., :1].contiguous()))
    if kind == 'ones':                        # c = N, m = 1: the unmasked values within the same bound
        y64, _ = _cpu(net, x, None, None, torch.float64)
        y32, _ = _cpu(net, x, None, None, torch.float32)
        with torch.no_grad():
            _check('mask ones vs no mask', dev(x.to(DEV), mask=mask.to(DEV)), y32, y64)


def test_a_fully_masked_set_is_nan_and_no_other_set_sees_it():
    net = _net(13, 4, [12, 9], 3, activation='Sigmoid').to(DEV)
    x = torch.randn(MB, MN, 4, generator=ph.generator('mask-x')).to(DEV)
    mask = _mask('binary').to(DEV)
    dead = mask.clone()
    dead[2] = 0.0
    other = mask.clone()
    other[2] = 1.0
    with torch.no_grad():
        y, want = net(x, mask=dead), net(x, mask=other)
    assert net._last_path == 'kernel'
    assert torch.isnan(y[2]).all()
    keep = [i for i in range(MB) if i != 2]
    assert not torch.isnan(y[keep]).any() and torch.equal(y[keep], want[keep])


def _ten_sets():
    net = _net(14, 5, [24], 6, final_activation='Tanh')
    g = ph.generator('ten-sets')
    return net, torch.randn(10, 33, 5, generator=g), torch.randn(10, 33, 6, generator=g)


def test_set_independence_bitwise_and_equivariance():
    net, x, gy = _ten_sets()
    dev = copy.deepcopy(net).to(DEV)
    y, grads, path = _gpu(dev, x.to(DEV), None, gy.to(DEV))
    assert path == 'kernel'
    for s in range(10):
        ys, gs, _ = _gpu(dev, x[s:s + 1].to(DEV), None, gy[s:s + 1].to(DEV))
        assert torch.equal(ys[0], y[s]) and torch.equal(gs[0][0], grads[0][s]), s
    perm = torch.randperm(33, generator=ph.generator('perm'))
    xp = x[:, perm]
    y64, _ = _cpu(net, xp, None, None, torch.float64)
    y32, _ = _cpu(net, xp, None, None, torch.float32)
    _check('permuted elements', y[:, perm], y32, y64)
    with torch.no_grad():
        _check('permuted input', dev(xp.to(DEV)), y32, y64)


def test_two_calls_give_the_same_bits():
    net, x, gy = _ten_sets()
    dev = copy.deepcopy(net).to(DEV)
    mask = (torch.rand(10, 33, 1, generator=ph.generator('det-mask')) < 0.8).float().to(DEV)
    for mk in (None, mask):
        y1, g1, path = _gpu(dev, x.to(DEV), mk, gy.to(DEV))
        y2, g2, _ = _gpu(dev, x.to(DEV), mk, gy.to(DEV))
        assert path == 'kernel'
        assert torch.equal(y1, y2)
        for name, a, b in zip(NAMES, g1, g2):
            assert torch.equal(a, b), name


@pytest.mark.parametrize('layout', ['bf16', 'row_strided', 'odd_offset', 'strided_columns'])
def test_input_layouts(layout, monkeypatch):
    net = _net(15, 6, [10], 4)
    B, N, D = 5, 9, 6
    g = ph.generator('layouts')
    x = torch.randn(B, N, D, generator=g)
    gy = torch.randn(B, N, 4, generator=g)
    if layout == 'bf16':
        x = x.to(torch.bfloat16).float()                 # the values a bf16 tensor holds
    y32, g32 = _cpu(net, x, None, gy, torch.float32)
    y64, g64 = _cpu(net, x, None, gy, torch.float64)
    dev = copy.deepcopy(net).to(DEV)
    if layout == 'bf16':
        xd = x.to(DEV).to(torch.bfloat16)
    elif layout == 'row_strided':
        wide = torch.full((B, N, D + 5), float('nan'), device=DEV)
        wide[..., :D] = x.to(DEV)
        xd = wide[..., :D]
        assert not xd.is_contiguous() and xd.stride(-1) == 1
    elif layout == 'odd_offset':
        flat = torch.full((B * N * D + 3,), float('nan'), device=DEV)
        flat[1:1 + B * N * D] = x.to(DEV).reshape(-1)
        xd = flat[1:1 + B * N * D].view(B, N, D)
        assert xd.storage_offset() == 1
    else:
        pairs = torch.full((B, N, D, 2), float('nan'), device=DEV)
        pairs[..., 0] = x.to(DEV)
        xd = pairs[..., 0]
        assert xd.stride(-1) == 2
    ph.poison_outputs(monkeypatch, DEV)
    xd = xd.detach().requires_grad_(True)
    y = dev(xd)
    assert dev._last_path == 'kernel' and y.dtype == torch.float32
    dx, = torch.autograd.grad(y, xd, gy.to(DEV))
    assert dx.dtype == xd.dtype and dx.shape == xd.shape
    _check(f'{layout} y', y, y32, y64)
    if layout == 'bf16':                                  # the cast's backward rounds dx to bf16: 2^-9 relative on top
        assert (dx.float().cpu().double() - g64[0]).abs().max().item() <= 2.0 ** -8 * g64[0].abs().max().item()
    else:
        _check(f'{layout} dx', dx, g32[0], g64[0])


def test_pass_loop():
    """Every workgroup takes a second trip round its pass loop: y and dx repeat the period's bits, the parameter gradients are the
    period's scaled by the tiling."""
    N = 33
    net = _net(16, 4, [8], 3)
    g = ph.generator('pass-loop')
    xs, gs = torch.randn(ph.SET_PERIOD, N, 4, generator=g), torch.randn(ph.SET_PERIOD, N, 3, generator=g)
    n_sets = ph.big_sets(DEV, N)
    ph.assert_multi_pass(n_sets * N, N, DEV)
    dev = copy.deepcopy(net).to(DEV)
    y_small, g_small, _ = _gpu(dev, xs.to(DEV), None, gs.to(DEV))
    y, grads, path = _gpu(dev, ph.tile(xs.to(DEV), n_sets), None, ph.tile(gs.to(DEV), n_sets))
    assert path == 'kernel'
    ph.assert_tiled('y', y, y_small)
    ph.assert_tiled('dx', grads[0], g_small[0])
    q, rem = divmod(n_sets, ph.SET_PERIOD)

    def scaled(dtype):
        whole = _cpu(net, xs, None, gs, dtype)[1][1:]
        part = _cpu(net, xs[:rem], None, gs[:rem], dtype)[1][1:]
        return [q * a + b for a, b in zip(whole, part)]
    for name, got, ref, truth in zip(NAMES[1:], grads[1:], scaled(torch.float32), scaled(torch.float64)):
        _check(f'pass loop {name}', got, ref, truth)


def test_gates():
    net = _net(17, 4, [8], 3).to(DEV)
    x = torch.randn(3, 5, 4, device=DEV, requires_grad=True)
    g1, = torch.autograd.grad(net(x).sum(), x, create_graph=True)
    assert net._last_path == 'kernel'
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g1.sum(), x)
    g1, = torch.autograd.grad(net.forward_twice_differentiable(x).tanh().sum(), x, create_graph=True)
    assert torch.autograd.grad(g1.sum(), x)[0].shape == x.shape
    mask = torch.ones(3, 5, 1, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError):
        net(x, mask=mask)
    with torch.no_grad():
        assert net(x, mask=mask).shape == (3, 5, 3)
    # an empty batch and a subclass run the composed sequence
    assert net(torch.zeros(0, 5, 4, device=DEV)).shape == (0, 5, 3) and net._last_path == 'composed'

    class Sub(EquivariantNet):
        pass
    sub = Sub(4, [8], 3).to(DEV)
    with torch.no_grad():
        sub(x)
    assert sub._last_path == 'composed'


def test_set_data_coupling_over_the_net():
    torch.manual_seed(18)
    B, N, D, L = 3, 6, 4, 2
    net = EquivariantNet(D + L, [16], 2 * D)
    f = st.Coupling(st.Affine(D, latent_net=net), mask='ordered_left_half', set_data=True).to(DEV)
    net = f.transform.latent_net
    x, latent = torch.randn(B, N, D, device=DEV), torch.randn(B, N, L, device=DEV)
    m = st.util.get_mask('ordered_left_half')(N).to(DEV).unsqueeze(-1).expand(B, N, D)

    def formula(n, xx, mm, lat):
        ls, shift = n.forward_twice_differentiable(torch.cat([xx * mm, lat], -1)).chunk(2, -1)
        return (xx * torch.exp(ls) + shift) * (1 - mm) + xx * mm, (ls * (1 - mm)).sum(-1, keepdim=True)
    n64 = copy.deepcopy(net).cpu().double()
    y64, l64 = formula(n64, x.cpu().double(), m.cpu().double(), latent.cpu().double())
    (y64.sum() + l64.sum()).backward()
    n32 = copy.deepcopy(net).cpu()
    y32, l32 = formula(n32, x.cpu(), m.cpu(), latent.cpu())
    (y32.sum() + l32.sum()).backward()
    with torch.no_grad():
        y, ldj = f.forward_and_log_det_jacobian(x, latent=latent)
        assert net._last_path == 'kernel'
        _check('coupling y', y, y32.detach(), y64.detach())
        _check('coupling ldj', ldj, l32.detach(), l64.detach())
        back = f.inverse(y, latent=latent)
        assert net._last_path == 'kernel'
        assert (back - x).abs().max().item() <= 1e-4
    net._last_path = None
    y, ldj = f.forward_and_log_det_jacobian(x, latent=latent)
    assert y.requires_grad and net._last_path == 'kernel'
    _check('coupling y [graph]', y, y32.detach(), y64.detach())
    _check('coupling ldj [graph]', ldj, l32.detach(), l64.detach())
    (y.sum() + ldj.sum()).backward()
    for name, p, p32, p64 in zip(NAMES[1:], _params(net), _params(n32), _params(n64)):
        _check(f'coupling {name}', p.grad, p32.grad, p64.grad)


def test_cnf_paths_never_see_the_kernel(monkeypatch):
    f = sh.make(3, [16, 8]).to(DEV)
    net = f.odefunc.diffeq.net
    x = torch.randn(4, 5, 3, device=DEV)

    def forbidden(self, *a, **k):
        raise AssertionError('ContinuousTransform called EquivariantNet.forward')
    with torch.no_grad():
        want_y, want_l = f.forward_and_log_det_jacobian(x)
    assert f._last_path == 'kernel' and net._last_path is None
    ref_y, ref_l = f._composed_reference(x, None)
    assert net._last_path is None
    monkeypatch.setattr(EquivariantNet, 'forward', forbidden)
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(x)
    again_y, again_l = f._composed_reference(x, None)
    assert torch.equal(y, want_y) and torch.equal(l, want_l)
    assert torch.equal(again_y, ref_y) and torch.equal(again_l, ref_l)
    assert net._last_path is None
