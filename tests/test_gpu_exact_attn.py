"""GPU: ContinuousTransform(divergence='exact') over DiffeqExactTraceAttention -- sx_cnf_exact_attn_flow against fixture F22, the
composition path, the kernel's shape edges, instantiations, activations and heads, set independence, slot invariance, equivariance,
twins, the non-finite rule, round trips, storage, the image cache, coverage gates, and training through the composition path.

Tolerances are cnfhelp.bound's: e_ref = max |fp32 sequence - fp64| is the fp32 sequence's own error against the fp64 restatement of
the same grid (exactattnhelp.solve64 over closed_form_attn); the kernel must stay within 8 e_ref (floor 1e-6 * max(1, max |fp64|)).
The fp32 sequence is the fixture where F22 holds the case and exactattnhelp.solve32 elsewhere."""
import pytest
import torch

import stribor_amd as st

import cnfhelp as ch
import exactattnhelp as xh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


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


def _check(f, x, lat=None, want_path='kernel', reverse=False, mask=None):
    """forward_and_log_det_jacobian on the GPU against the fp64 solve, bounded by the fp32 restatement's own error."""
    f = f.cpu()
    y64, l64 = xh.solve64(f, x, lat, reverse)
    y32, l32 = xh.solve32(f, x, lat, reverse)
    f = f.to(DEV)
    kw = {} if lat is None else {'latent': lat.to(DEV)}
    if mask is not None:
        kw['mask'] = mask.to(DEV)
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(x.to(DEV), reverse=reverse, **kw)
    assert f._last_path == want_path
    _close('y', y, y32, y64)
    _close('ldj', l, l32, l64)
    return y, l


EDGES = {
    # name: (shape, hidden, d_h, latent, heads)
    'n1_no_exchange': ((5, 1, 3), [16], 3, 0, 2),
    'n2_one_key_per_query': ((4, 2, 3), [16, 8], 3, 0, 1),
    'n3': ((3, 3, 2), [24], 2, 2, 4),
    'n32_one_wave_per_set': ((2, 32, 2), [16], 3, 0, 2),
    'n33_straddles_waves': ((2, 33, 3), [20, 16], 4, 0, 4),
    'all_padding_wave': ((1, 43, 2), [16], 3, 0, 1),
    'n128_one_set_per_workgroup': ((2, 128, 2), [16], 2, 0, 2),
    'two_workgroups_ragged': ((30, 5, 2), [16, 16], 3, 3, 4),
    'dim1_query_is_its_bias': ((4, 5, 1), [12, 8], 3, 0, 2),
    'dim8_four_query_tiles': ((3, 5, 8), [32, 16], 4, 0, 2),
    'largest_mandated_image': ((3, 5, 2), [64, 32], 8, 0, 4),
    'd_h1': ((4, 3, 3), [28], 1, 0, 1),
    'latent40_two_tiles': ((3, 4, 2), [16], 5, 40, 2),
    'no_rows': ((0, 4, 2), [16], 3, 0, 1),
}


@pytest.mark.parametrize('solver', ['rk4', 'midpoint'])
@pytest.mark.parametrize('name', sorted(EDGES))
def test_shape_edges(name, solver):
    shp, hidden, d_h, latent, heads = EDGES[name]
    f = xh.make(shp[-1], hidden, d_h, latent=latent, heads=heads, solver=solver, T=0.7, seed=sum(map(ord, name)))
    x = torch.randn(*shp)
    lat = torch.randn(*shp[:-1], latent) if latent else None
    for reverse in (False, True):
        _check(f, x, lat, 'kernel', reverse=reverse)


# the kernel's instantiations (sx_cnf_exact_attn_flow's dispatch): hidden tiles x hidden layers x output tiles; one hidden layer is the
# embedding alone, <= 32 wide, so (2, 1, .) does not exist.  The heads are a run-time loop of every instantiation.
INSTANTIATIONS = [(1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 2, 1), (1, 2, 2), (1, 2, 4), (2, 2, 1), (2, 2, 2), (2, 2, 4)]
TILE_TRIPLES = {
    # (HT, NH, OT, heads): (hidden, d_h) that selects it
    (1, 1, 1, 1): ([20], 1), (1, 1, 2, 2): ([20], 3), (1, 1, 4, 4): ([20], 5),
    (1, 2, 1, 4): ([20, 12], 2), (1, 2, 2, 1): ([32, 20], 4), (1, 2, 4, 2): ([20, 20], 8),
    (2, 2, 1, 2): ([33, 20], 1), (2, 2, 2, 4): ([64, 20], 3), (2, 2, 4, 1): ([40, 20], 5),
}
assert sorted(t[:3] for t in TILE_TRIPLES) == INSTANTIATIONS and {t[3] for t in TILE_TRIPLES} == {1, 2, 4}
assert all((max(1 if w <= 32 else 2 for w in hidden), len(hidden), 1 if d_h <= 2 else 2 if d_h <= 4 else 4) == triple[:3]
           for triple, (hidden, d_h) in TILE_TRIPLES.items())


@pytest.mark.parametrize('triple', sorted(TILE_TRIPLES))
def test_every_kernel_instantiation(triple):
    hidden, d_h = TILE_TRIPLES[triple]
    f = xh.make(3, hidden, d_h, heads=triple[3], seed=sum(triple) + 10 * len(hidden))
    _check(f, torch.randn(3, 5, 3), None, 'kernel')


@pytest.mark.parametrize('act', ['Identity', 'Tanh', 'ReLU', 'Sigmoid', 'ELU', 'Softplus', 'LeakyReLU'])
def test_activations(act):
    f = xh.make(3, [24, 16], 3, latent=2, heads=2, seed=7)
    xh.set_activation(f.odefunc.diffeq, act)
    _check(f, torch.randn(6, 7, 3), torch.randn(6, 7, 2), 'kernel')


@pytest.mark.parametrize('E', [8, 32])
@pytest.mark.parametrize('heads', [1, 2, 4])
def test_heads(heads, E):
    f = xh.make(4, [20, E], 3, heads=heads, seed=8 + heads)
    _check(f, torch.randn(7, 9, 4), None, 'kernel')


def test_twins_get_equal_outputs():
    f = xh.make(3, [16, 16], 4, latent=2, heads=2, seed=9)
    x, lat = torch.randn(4, 6, 3), torch.randn(4, 6, 2)
    x[:, 4], lat[:, 4] = x[:, 1], lat[:, 1]
    y, l = _check(f, x, lat, 'kernel')
    # element 1 sees key 4 where element 4 sees key 1: the same keys at other positions of the sweep, so the sums round differently and
    # the twins are not bit-equal.  In exact arithmetic they are equal, so each is within the bound of ONE truth: twice the bound apart
    tol_y = 2 * ch.bound(xh.solve32(f.cpu(), x, lat)[0], xh.solve64(f, x, lat)[0])[0]
    tol_l = 2 * ch.bound(xh.solve32(f, x, lat)[1], xh.solve64(f, x, lat)[1])[0]
    assert (y[:, 4] - y[:, 1]).abs().max().item() <= tol_y and (l[:, 4] - l[:, 1]).abs().max().item() <= tol_l
    y64 = xh.solve64(f, x, lat)[0]
    assert torch.equal(y64[:, 4], y64[:, 1]) or (y64[:, 4] - y64[:, 1]).abs().max().item() <= 1e-13


@pytest.mark.parametrize('n', [5, 33, 128])
def test_set_independence_and_slot_invariance(n):
    f = xh.make(2, [16], 3, latent=1, heads=2, seed=n).to(DEV)
    B = 40 if n == 5 else 5
    x, lat = torch.randn(B, n, 2, device=DEV), torch.randn(B, n, 1, device=DEV)
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(x, latent=lat)
        x2 = x.clone()
        x2[2] = torch.randn(n, 2, device=DEV)
        y2, l2 = f.forward_and_log_det_jacobian(x2, latent=lat)
        perm = torch.roll(torch.arange(B), 3)                        # every set moves to another slot (n = 5: across workgroups too)
        yp, lp = f.forward_and_log_det_jacobian(x[perm], latent=lat[perm])
        ya, la = f.forward_and_log_det_jacobian(x[1:2], latent=lat[1:2])          # a set solved alone
    assert f._last_path == 'kernel'
    keep = [b for b in range(B) if b != 2]
    assert torch.equal(y[keep], y2[keep]) and torch.equal(l[keep], l2[keep]) and not torch.equal(y[2], y2[2])
    assert torch.equal(yp, y[perm]) and torch.equal(lp, l[perm])
    assert torch.equal(ya[0], y[1]) and torch.equal(la[0], l[1])


def test_equivariance():
    f = xh.make(3, [16, 16], 3, latent=2, heads=4, seed=11)
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


@pytest.mark.parametrize('n', [6, 40])
def test_a_nan_element_poisons_its_set_alone(n):
    f = xh.make(2, [16, 8], 3, heads=2, seed=17).to(DEV)
    x = torch.randn(9, n, 2, device=DEV)
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(x)
        x2 = x.clone()
        x2[4, 3, 1] = float('nan')
        y2, l2 = f.forward_and_log_det_jacobian(x2)
    assert f._last_path == 'kernel'
    keep = [b for b in range(9) if b != 4]
    assert torch.isnan(y2[4]).all() and torch.isnan(l2[4]).all()
    assert torch.equal(y2[keep], y[keep]) and torch.equal(l2[keep], l[keep])


def test_single_outputs_round_trip_and_log_det_consistency():
    f = xh.make(3, [32, 16], 3, latent=2, heads=2, step=1 / 16, seed=12)
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


def test_bf16_and_unaligned_inputs():
    f = xh.make(3, [16, 8], 3, latent=2, heads=2, seed=18).to(DEV)
    x, lat = torch.randn(6, 5, 3, device=DEV), torch.randn(6, 5, 2, device=DEV)
    with torch.no_grad():
        xb = x.to(torch.bfloat16)
        yb, lb = f.forward_and_log_det_jacobian(xb, latent=lat)
        yu, lu = f.forward_and_log_det_jacobian(xb.float(), latent=lat)
        assert f._last_path == 'kernel' and yb.dtype == torch.bfloat16 and lb.dtype == torch.float32
        assert torch.equal(yb, yu.to(torch.bfloat16)) and torch.equal(lb, lu)
        y, l = f.forward_and_log_det_jacobian(x, latent=lat)
        buf = torch.empty(x.numel() + 1, device=DEV)
        view = buf[1:].view_as(x)                                     # 4 bytes past a 16-byte boundary
        view.copy_(x)
        lbuf = torch.empty(lat.numel() + 1, device=DEV)
        lview = lbuf[1:].view_as(lat)
        lview.copy_(lat)
        assert view.data_ptr() % 16 == 4
        yv, lv = f.forward_and_log_det_jacobian(view, latent=lview)
    assert f._last_path == 'kernel' and torch.equal(yv, y) and torch.equal(lv, l)


def test_cache_follows_weights_and_masks():
    f = xh.make(3, [24, 16], 3, latent=2, heads=2, seed=15).to(DEV)
    x, lat = torch.randn(6, 5, 3, device=DEV), torch.randn(6, 5, 2, device=DEV)

    def fresh():
        g = xh.make(3, [24, 16], 3, latent=2, heads=2, seed=99).to(DEV)
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
    q = f.odefunc.diffeq.exclusive_net.q
    with torch.no_grad():
        last = q.masked_linears()[-1]
        i, j = [int(v[0]) for v in torch.nonzero(last.mask, as_tuple=True)]
        last.mask[i, j] = 0                                           # a manual edit of one entry of a mask buffer
        y2, l2 = f.forward_and_log_det_jacobian(x, latent=lat)
    assert f._last_path == 'kernel' and not torch.equal(y1, y2)
    yb, lb = fresh()
    assert torch.equal(y2, yb) and torch.equal(l2, lb)


@pytest.mark.parametrize('edge', ['heads8', 'e33', 'mask'])
def test_out_of_coverage_runs_composed(edge):
    hidden = [33] if edge == 'e33' else [16]
    f = xh.make(2, hidden, 2, heads=8 if edge == 'heads8' else 1, seed=13)
    x = torch.randn(2, 4, 2)
    mask = (torch.rand(2, 4, 1) > 0.3).float() if edge == 'mask' else None          # (the net never sees it; the path must still switch)
    _check(f, x, None, 'composed', mask=mask)
    if edge == 'mask':
        with torch.no_grad():
            f.forward_and_log_det_jacobian(x.to(DEV))
        assert f._last_path == 'kernel'                               # the same module and sets without a mask


def test_training_through_the_composition_path():
    f = xh.make(2, [16, 8], 2, latent=1, heads=2, seed=16).to(DEV).train()
    x, lat = torch.randn(6, 4, 2, device=DEV), torch.randn(6, 4, 1, device=DEV)
    y, ldj = f.forward_and_log_det_jacobian(x, latent=lat)
    assert f._last_path == 'composed' and ldj.requires_grad and ldj.shape == (6, 4, 1)
    (-ldj.mean()).backward()
    net = f.odefunc.diffeq
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    for part in (net.exclusive_net.q, net.exclusive_net.k, net.exclusive_net.v, net.exclusive_net.proj, net.dimwise_net):
        assert sum(p.grad.abs().sum().item() for p in part.parameters()) > 0
    with torch.no_grad():
        yk, lk = f.eval().forward_and_log_det_jacobian(x, latent=lat)
    assert f._last_path == 'kernel'
    tol = 1e-4 * max(1.0, y.abs().max().item(), ldj.abs().max().item())
    assert (yk - y.detach()).abs().max().item() <= tol and (lk - ldj.detach()).abs().max().item() <= tol
