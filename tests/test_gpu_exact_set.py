"""GPU: ContinuousTransform(divergence='exact') over DiffeqExactTraceDeepSet -- sx_cnf_exact_set_flow against fixture F19, the
composition path, the kernel's shape edges, activations and poolings, ties, set independence, slot invariance, equivariance, round
trips, coverage gates, the image cache, and training through the composition path.

Tolerances are cnfhelp.bound's: e_ref = max |fp32 sequence - fp64| is the fp32 sequence's own error against the fp64 restatement of
the same grid (exactsethelp.solve64 over closed_form_set); the kernel must stay within 8 e_ref (floor 1e-6 * max(1, max |fp64|)).
The fp32 sequence is the fixture where F19 holds the case and exactsethelp.solve32 elsewhere."""
import copy
import math

import pytest
import torch
import torch.nn as nn

import stribor_amd as st

import cnfhelp as ch
import exactsethelp as xh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(t):
    return None if t is None else t.to(DEV)


def _close(what, got, ref32, truth):
    tol, e_ref = ch.bound(ref32, truth)
    err = (got.cpu().double() - truth).abs().max().item() if truth.numel() else 0.0
    print(f'{what}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e}')
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    assert err <= tol, (what, err, e_ref, tol)


def _run_case(case, path):
    g = xh.golden()
    f, x, lat, m = xh.build_case(case)
    y64, l64 = xh.solve64(f, x, lat)
    xb64, lb64 = xh.solve64(f, g.t(f'{case}/y'), lat, reverse=True)
    f = f.to(DEV)
    kw = {} if lat is None else {'latent': lat.to(DEV)}
    if path == 'kernel':
        with torch.no_grad():
            y, l = f.forward_and_log_det_jacobian(x.to(DEV), **kw)
            assert f._last_path == 'kernel', case
            assert f._num_evals() == m['num_evals']
            xb, lb = f.inverse_and_log_det_jacobian(g.t(f'{case}/y').to(DEV), **kw)
            assert f._last_path == 'kernel', case
            assert f._num_evals() == m['num_evals']
    else:
        y, l = f._composed_reference(x.to(DEV), kw.get('latent'))
        xb, lb = f._composed_reference(g.t(f'{case}/y').to(DEV), kw.get('latent'), reverse=True)
    for name, got, truth in (('y', y, y64), ('ldj', l, l64), ('x_back', xb, xb64), ('ldj_back', lb, lb64)):
        _close(f'{case} [{path}] {name}', got, g.t(f'{case}/{name}'), truth)


@pytest.mark.parametrize('case', xh.case_names())
def test_golden_parity_kernel(case):
    _run_case(case, 'kernel')


@pytest.mark.parametrize('case', [c for c in xh.case_names() if '/rk4/T0.7/' in c])
def test_paths_agree(case):
    _run_case(case, 'composed')


def _check(f, x, lat=None, want_path='kernel', reverse=False, mask=None, graph=False):
    """forward_and_log_det_jacobian on the GPU against the fp64 solve, bounded by the fp32 restatement's own error."""
    f = f.cpu()
    y64, l64 = xh.solve64(f, x, lat, reverse)
    y32, l32 = xh.solve32(f, x, lat, reverse)
    f = f.to(DEV)
    kw = {} if lat is None else {'latent': lat.to(DEV)}
    if mask is not None:
        kw['mask'] = mask.to(DEV)
    with torch.set_grad_enabled(graph):
        y, l = f.forward_and_log_det_jacobian(x.to(DEV).requires_grad_(graph), reverse=reverse, **kw)
    assert f._last_path == want_path
    _close('y', y.detach(), y32, y64)
    _close('ldj', l.detach(), l32, l64)
    return y.detach(), l.detach()


EDGES = {
    # name: (shape, hidden, d_h, latent, pooling)
    'n1_no_exchange': ((5, 1, 3), [16], 3, 0, 'max'),
    'n2_max_second_value': ((4, 2, 3), [16, 24], 3, 0, 'max'),
    'n3': ((3, 3, 2), [24], 2, 2, 'mean'),
    'n32_one_wave_per_set': ((2, 32, 2), [16], 3, 0, 'sum'),
    'n33_straddles_waves': ((2, 33, 3), [20, 16], 4, 0, 'max'),
    'all_padding_wave': ((1, 43, 2), [16], 3, 0, 'mean'),
    'n128_one_set_per_workgroup': ((2, 128, 2), [16], 2, 0, 'sum'),
    'two_workgroups_ragged': ((30, 5, 2), [16, 16], 3, 3, 'max'),
    'largest_image': ((3, 5, 16), [64, 64], 8, 0, 'max'),
    'd_h1': ((4, 3, 3), [40], 1, 0, 'sum'),
    'latent40_two_tiles': ((3, 4, 2), [16], 5, 40, 'mean'),
    'no_rows': ((0, 4, 2), [16], 3, 0, 'max'),
}


@pytest.mark.parametrize('solver', ['rk4', 'midpoint'])
@pytest.mark.parametrize('name', sorted(EDGES))
def test_shape_edges(name, solver):
    shp, hidden, d_h, latent, pooling = EDGES[name]
    f = xh.make(shp[-1], hidden, d_h, latent=latent, pooling=pooling, solver=solver, T=0.7, seed=sum(map(ord, name)))
    x = torch.randn(*shp)
    lat = torch.randn(*shp[:-1], latent) if latent else None
    for reverse in (False, True):
        _check(f, x, lat, 'kernel', reverse=reverse)


TILE_TRIPLES = {
    # the kernel instantiation (HT, NH, OT): (hidden, d_h) that selects it
    (1, 1, 1): ([20], 1), (1, 1, 2): ([20], 3), (1, 1, 4): ([20], 5),
    (1, 2, 1): ([20, 20], 1), (1, 2, 2): ([20, 20], 3), (1, 2, 4): ([20, 20], 5),
    (2, 1, 1): ([33], 1), (2, 1, 2): ([33], 3), (2, 1, 4): ([33], 5),
    (2, 2, 1): ([20, 33], 1), (2, 2, 2): ([33, 20], 3), (2, 2, 4): ([33, 33], 5),
}
assert set(TILE_TRIPLES) == {(ht, nh, ot) for ht in (1, 2) for nh in (1, 2) for ot in (1, 2, 4)}
assert all((max(1 if w <= 32 else 2 for w in hidden), len(hidden), 1 if d_h <= 2 else 2 if d_h <= 4 else 4) == triple
           for triple, (hidden, d_h) in TILE_TRIPLES.items())


@pytest.mark.parametrize('triple', sorted(TILE_TRIPLES))
def test_every_kernel_instantiation(triple):
    hidden, d_h = TILE_TRIPLES[triple]
    f = xh.make(3, hidden, d_h, pooling='max', seed=sum(triple) + 10 * len(hidden))
    _check(f, torch.randn(3, 5, 3), None, 'kernel')


@pytest.mark.parametrize('act', ['Identity', 'Tanh', 'ReLU', 'Sigmoid', 'ELU', 'Softplus', 'LeakyReLU'])
def test_activations(act):
    f = xh.make(3, [24, 16], 3, latent=2, pooling='mean', seed=7)
    xh.set_activation(f.odefunc.diffeq, act)
    _check(f, torch.randn(6, 7, 3), torch.randn(6, 7, 2), 'kernel')


@pytest.mark.parametrize('hidden', [[40], [20, 33]])
@pytest.mark.parametrize('pooling', ['max', 'mean', 'sum'])
def test_poolings(pooling, hidden):
    f = xh.make(4, hidden, 5, pooling=pooling, seed=8)
    _check(f, torch.randn(7, 9, 4), None, 'kernel')


def test_ties_in_max_pooling():
    f = xh.make(3, [16, 16], 4, latent=2, pooling='max', seed=9)
    x, lat = torch.randn(4, 6, 3), torch.randn(4, 6, 2)
    x[:, 4], lat[:, 4] = x[:, 1], lat[:, 1]                           # twins: every column of their embeddings ties
    y, l = _check(f, x, lat, 'kernel')
    assert torch.equal(y[:, 4], y[:, 1]) and torch.equal(l[:, 4], l[:, 1])


@pytest.mark.parametrize('n', [5, 33, 128])
@pytest.mark.parametrize('pooling', ['max', 'sum'])
def test_set_independence_and_slot_invariance(n, pooling):
    f = xh.make(2, [16], 3, latent=1, pooling=pooling, seed=n).to(DEV)
    B = 40 if n == 5 else 5
    x, lat = torch.randn(B, n, 2, device=DEV), torch.randn(B, n, 1, device=DEV)
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(x, latent=lat)
        x2 = x.clone()
        x2[2] = torch.randn(n, 2, device=DEV)
        y2, l2 = f.forward_and_log_det_jacobian(x2, latent=lat)
        perm = torch.roll(torch.arange(B), 3)                        # every set moves to another slot (n = 5: across workgroups too)
        yp, lp = f.forward_and_log_det_jacobian(x[perm], latent=lat[perm])
    assert f._last_path == 'kernel'
    keep = [b for b in range(B) if b != 2]
    assert torch.equal(y[keep], y2[keep]) and torch.equal(l[keep], l2[keep]) and not torch.equal(y[2], y2[2])
    assert torch.equal(yp, y[perm]) and torch.equal(lp, l[perm])


@pytest.mark.parametrize('pooling', ['max', 'mean', 'sum'])
def test_equivariance(pooling):
    f = xh.make(3, [16, 16], 3, latent=2, pooling=pooling, seed=11)
    x, lat = torch.randn(3, 37, 3), torch.randn(3, 37, 2)
    perm = torch.randperm(37)
    y64, l64 = xh.solve64(f, x, lat)
    y32, l32 = xh.solve32(f, x, lat)
    f = f.to(DEV)
    with torch.no_grad():
        yp, lp = f.forward_and_log_det_jacobian(x[:, perm].to(DEV), latent=lat[:, perm].to(DEV))
    assert f._last_path == 'kernel'
    _close('y', yp, y32[:, perm], y64[:, perm])
    _close('ldj', lp, l32[:, perm], l64[:, perm])


def test_single_outputs_round_trip_and_log_det_consistency():
    f = xh.make(3, [32], 3, latent=2, pooling='mean', step=1 / 16, seed=12)
    x, lat = torch.randn(5, 9, 3), torch.randn(5, 9, 2)
    y32, l32 = xh.solve32(f, x, lat)
    xb32, lb32 = xh.solve32(f, y32, lat, reverse=True)
    e_rt = (xb32 - x).abs().max().item()                             # the fp32 sequence's own round-trip error (grid + fp32)
    e_ld = (l32 + lb32).abs().max().item()
    f = f.to(DEV)
    xd, kw = x.to(DEV), {'latent': lat.to(DEV)}
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(xd, **kw)
        assert torch.equal(f(xd, **kw), y) and f._last_path == 'kernel'          # (the call without a log-det skips the tangent)
        assert torch.equal(f.log_det_jacobian(xd, y, **kw), l)
        xb, lb = f.inverse_and_log_det_jacobian(y, **kw)
        assert torch.equal(f.inverse(y, **kw), xb) and f._last_path == 'kernel'
    rt = (xb.cpu() - x).abs().max().item()
    ld = (l + lb).abs().max().item()
    print(f'round trip {rt:.3e} (fp32 sequence {e_rt:.3e}), ldj + ldj_back {ld:.3e} (fp32 sequence {e_ld:.3e})')
    assert rt <= max(8 * e_rt, 1e-6 * max(1.0, x.abs().max().item()))
    assert ld <= max(8 * e_ld, 1e-6 * max(1.0, l.abs().max().item()))


@pytest.mark.parametrize('edge', ['n129', 'hidden65', 'dim17', 'd_h9', 'mask', 'graph', 'mixed_activation', 'activation_parameters', 'hand_built'])
def test_coverage_gate_takes_the_composition_path(edge):
    dim = 17 if edge == 'dim17' else 2
    hidden = [65] if edge == 'hidden65' else [16]
    d_h = 9 if edge == 'd_h9' else 2
    n = 129 if edge == 'n129' else 4
    f = xh.make(dim, hidden, d_h, pooling='max', seed=13)
    net = f.odefunc.diffeq
    if edge == 'mixed_activation':
        net.exclusive_net.interaction.set_emb.net.net[1] = nn.Sigmoid()
    elif edge == 'activation_parameters':
        xh.set_activation(net, 'LeakyReLU', lambda: nn.LeakyReLU(0.2))
    elif edge == 'hand_built':
        f = xh.make(dim, hidden, d_h, net=st.net.DiffeqExactTrace(net.exclusive_net, net.dimwise_net), biases=False)
    x = torch.randn(2, n, dim)
    mask = (torch.rand(2, n, 1) > 0.3).float() if edge == 'mask' else None          # (these nets ignore it; the path must still switch)
    if edge in ('mixed_activation', 'activation_parameters', 'hand_built'):
        # closed_form_set restates the plain instance only: the module's own composition path in fp64 on the CPU is the truth here
        g64 = copy.deepcopy(f).double()
        name, step, grid = g64._grid(False)
        y64, l64 = g64._solve_composed(x.double(), None, None, name, grid, False)
        g32 = copy.deepcopy(f)
        y32, l32 = g32._solve_composed(x, None, None, name, grid, False)
        f = f.to(DEV)
        with torch.no_grad():
            y, l = f.forward_and_log_det_jacobian(x.to(DEV))
        assert f._last_path == 'composed'
        _close('y', y, y32, y64)
        _close('ldj', l, l32, l64)
        return
    _check(f, x, None, 'composed', mask=mask, graph=edge == 'graph')
    if edge in ('mask', 'graph'):
        with torch.no_grad():
            f.forward_and_log_det_jacobian(x.to(DEV))
        assert f._last_path == 'kernel'                               # the same module and sets without a mask / graph


def test_zero_trace_deepset_alone_runs_composed_with_zero_log_det():
    torch.manual_seed(14)
    f = st.ContinuousTransform(3, net=st.net.DiffeqZeroTraceDeepSet(3, [16], 3, pooling='mean'), divergence='exact', solver='rk4',
                               solver_options={'step_size': 0.25}).eval().to(DEV)
    x = torch.randn(4, 5, 3, device=DEV)
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(x)
    assert f._last_path == 'composed' and f.set_data and l.shape == (4, 5, 1)
    assert torch.all(l == 0) and (y - x).abs().max().item() > 0


def test_cache_follows_weights_and_masks():
    f = xh.make(3, [24, 16], 3, latent=2, pooling='sum', seed=15).to(DEV)
    x, lat = torch.randn(6, 5, 3, device=DEV), torch.randn(6, 5, 2, device=DEV)

    def fresh():
        g = xh.make(3, [24, 16], 3, latent=2, pooling='sum', seed=99).to(DEV)
        g.load_state_dict(f.state_dict(), strict=True)
        with torch.no_grad():
            out = g.forward_and_log_det_jacobian(x, latent=lat)
        assert g._last_path == 'kernel'
        return out
    with torch.no_grad():
        y0, l0 = f.forward_and_log_det_jacobian(x, latent=lat)
        for p in f.parameters():
            p.mul_(1.25)                                              # an optimizer-style in-place update
        y1, l1 = f.forward_and_log_det_jacobian(x, latent=lat)
    assert f._last_path == 'kernel' and not torch.equal(y0, y1)
    ya, la = fresh()
    assert torch.equal(y1, ya) and torch.equal(l1, la)
    made = f.odefunc.diffeq.exclusive_net.elementwise
    with torch.no_grad():
        last = made.masked_linears()[-1]
        last.mask.copy_(1 - last.mask)                                # a manual edit of a mask buffer
        y2, l2 = f.forward_and_log_det_jacobian(x, latent=lat)
    assert f._last_path == 'kernel' and not torch.equal(y1, y2)
    yb, lb = fresh()
    assert torch.equal(y2, yb) and torch.equal(l2, lb)


@pytest.mark.parametrize('inside_flow', [False, True])
def test_training_gradients_against_fp64(inside_flow):
    """-log_prob.mean().backward() through the composition path against the same loss in fp64 on the CPU (the module's composition
    path on a double copy), at test_gpu_exact_trace.py's tolerance for the MLP instance: 1e-4 * max(1, max |.|)."""
    dim, shp = 2, (6, 4, 2)
    cnf = xh.make(dim, [16, 16], 2, latent=0, pooling='mean', seed=16)
    x = torch.randn(*shp)
    c64 = copy.deepcopy(cnf).double()
    name, step, grid = c64._grid(True)
    z, ldj = c64._solve_composed(x.double(), None, None, name, grid, True)
    lp64 = (-0.5 * z * z - 0.5 * math.log(2 * math.pi)).sum(-1, keepdim=True) + ldj
    loss64 = -lp64.mean()
    loss64.backward()
    cnf = cnf.to(DEV)
    if inside_flow:
        flow = st.NormalizingFlow(st.UnitNormal(dim), [cnf]).to(DEV)
        lp = flow.log_prob(x.to(DEV))
    else:
        zz, ll = cnf.inverse_and_log_det_jacobian(x.to(DEV))
        lp = (-0.5 * zz * zz - 0.5 * math.log(2 * math.pi)).sum(-1, keepdim=True) + ll
    assert cnf._last_path == 'composed' and lp.requires_grad and lp.shape == (*shp[:-1], 1)          # (the set axis is kept)
    loss = -lp.mean()
    loss.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-4 * max(1.0, abs(loss64.item()))
    want = dict(c64.odefunc.diffeq.named_parameters())
    for k, p in cnf.odefunc.diffeq.named_parameters():
        g64 = want[k].grad
        assert p.grad is not None and g64 is not None, k
        err = (p.grad.cpu().double() - g64).abs().max().item()
        assert err <= 1e-4 * max(1.0, g64.abs().max().item()), (k, err)
    assert sum(p.grad.abs().sum().item() for p in cnf.odefunc.diffeq.exclusive_net.parameters()) > 0
    with torch.no_grad():
        zk, lk = cnf.inverse_and_log_det_jacobian(x.to(DEV))
    assert cnf._last_path == 'kernel'
    lpk = (-0.5 * zk * zk - 0.5 * math.log(2 * math.pi)).sum(-1, keepdim=True) + lk
    assert abs(-lpk.mean().item() - loss.item()) <= 1e-4 * max(1.0, abs(loss.item()))
