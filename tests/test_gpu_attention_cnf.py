"""GPU: ContinuousTransform over sets with self attention -- sx_cnf_attn_flow against the reference's fixture F20, the composition
path, the shape edges of its set layout, set independence, equivariance, non-finite sets, the coverage gates, round trips and training.

Tolerances are cnfhelp.bound's: per case e_ref = max |fp32 sequence - fp64| is the fp32 sequence's own error against the fp64
restatement of the same grid (attnhelp.solve64, over the closed form of the divergence); the kernel must stay within 8 e_ref of the
fp64 values (floor 1e-6 * max(1, max |fp64|)).  The fp32 sequence is the fixture where F20 holds the case and attnhelp.solve32 (the
same restatement evaluated in fp32) elsewhere."""
import pytest
import torch

import stribor_amd as st

import attnhelp as ah
import cnfhelp as ch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _check(tag, got, ref, truth):
    tol, e_ref = ch.bound(ref, truth)
    err = (got.cpu().double() - truth).abs().max().item()
    print(f'{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e}')
    assert got.shape == truth.shape
    assert err <= tol, (tag, err, e_ref, tol)


def _run_case(case, path):
    g = ah.golden()
    f, x, lat, m = ah.build_case(case)
    y64, l64 = ah.solve64(f, x, lat)
    xb64, lb64 = ah.solve64(f, g.t(f'{case}/y'), lat, reverse=True)
    f = f.to(DEV)
    kw = {} if lat is None else {'latent': lat.to(DEV)}
    if path == 'kernel':
        with torch.no_grad():
            y, l = f.forward_and_log_det_jacobian(x.to(DEV), **kw)
            assert f._last_path == 'kernel', case
            assert f._num_evals() == m['num_evals']
            xb, lb = f.inverse_and_log_det_jacobian(g.t(f'{case}/y').to(DEV), **kw)
            assert f._last_path == 'kernel', case
    else:
        y, l = f._composed_reference(x.to(DEV), kw.get('latent'))
        xb, lb = f._composed_reference(g.t(f'{case}/y').to(DEV), kw.get('latent'), reverse=True)
    for name, got, truth in (('y', y, y64), ('ldj', l, l64), ('x_back', xb, xb64), ('ldj_back', lb, lb64)):
        _check(f'{case} [{path}] {name}', got, g.t(f'{case}/{name}'), truth)


@pytest.mark.parametrize('case', ah.case_names())
def test_golden_parity_kernel(case):
    _run_case(case, 'kernel')


@pytest.mark.parametrize('case', [c for c in ah.case_names() if '/rk4/T0.7/' in c])
def test_paths_agree(case):
    _run_case(case, 'composed')


def _both_ways(tag, f, x, lat=None):
    """Forward and reverse on the kernel against the fp64 restatement (fp32 sequence: attnhelp.solve32) -> the kernel's forward y, ldj."""
    y64, l64 = ah.solve64(f, x, lat)
    y32, l32 = ah.solve32(f, x, lat)
    xb64, lb64 = ah.solve64(f, y64.float(), lat, reverse=True)
    xb32, lb32 = ah.solve32(f, y64.float(), lat, reverse=True)
    f = f.to(DEV)
    kw = {} if lat is None else {'latent': lat.to(DEV)}
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(x.to(DEV), **kw)
        assert f._last_path == 'kernel', tag
        xb, lb = f.inverse_and_log_det_jacobian(y64.float().to(DEV), **kw)
        assert f._last_path == 'kernel', tag
    for name, got, ref, truth in (('y', y, y32, y64), ('ldj', l, l32, l64), ('x_back', xb, xb32, xb64), ('ldj_back', lb, lb32, lb64)):
        _check(f'{tag} {name}', got, ref, truth)
    return y, l


EDGE_CASES = {
    # name: ((B, N, dim), hidden_dim, n_heads, mask_diagonal, latent, activation)
    'n1': ((3, 1, 2), [8], 2, False, 0, None),
    'n1_fully_masked': ((3, 1, 2), [12, 8], 1, True, 0, 'Tanh'),
    'n2_one_key_per_query': ((5, 2, 2), [8], 1, True, 0, None),
    'n32_one_wave_per_set': ((2, 32, 3), [64, 32], 4, False, 0, 'Tanh'),
    'n33_straddles_waves': ((3, 33, 2), [24, 16], 2, True, 0, 'Sigmoid'),
    'n43_all_padding_wave': ((1, 43, 2), [16], 1, False, 0, None),
    'n128_one_set_per_workgroup': ((1, 128, 2), [40, 8], 2, False, 0, 'ELU'),
    'n128_masked': ((2, 128, 2), [8], 1, True, 0, None),
    'two_workgroups_ragged': ((30, 5, 2), [64, 32], 4, True, 0, 'LeakyReLU'),
    'head_width_1': ((4, 6, 2), [4], 4, False, 0, None),
    'head_width_1_deep': ((4, 6, 2), [5, 4], 4, True, 2, 'Softplus'),
    'largest_image': ((3, 20, 8), [64, 32], 4, False, 23, 'Tanh'),
    'dim1': ((4, 7, 1), [12, 8], 2, False, 0, 'ReLU'),
    'dim8': ((2, 9, 8), [32], 2, True, 0, None),
    'latent29': ((3, 6, 2), [12, 8], 1, False, 29, 'Identity'),
    'heads_across_groups': ((3, 5, 3), [12], 2, False, 1, None),
}


@pytest.mark.parametrize('name', sorted(EDGE_CASES))
@pytest.mark.parametrize('solver', ['rk4', 'midpoint'])
def test_shape_edges(name, solver):
    """The set layout's edges (set sizes around the wave and workgroup sizes, a ragged last workgroup, an all-padding wave), head
    widths 1 .. 32 (6: a head that ends inside an 8-feature group), both embedding depths at their widest, every offered activation,
    dim 1 and 8, a full input tile, non-zero biases everywhere: forward and reverse on the kernel against the fp64 restatement."""
    shape, hidden, heads, md, latent, act = EDGE_CASES[name]
    torch.manual_seed(sum(map(ord, name)))
    f = ah.make(shape[-1], hidden, n_heads=heads, mask_diagonal=md, latent=latent, T=0.7, solver=solver, act=act, biases=True)
    x = torch.randn(*shape)
    lat = torch.randn(*shape[:-1], latent) if latent else None
    y, l = _both_ways(f'{name}/{solver}', f, x, lat)
    if name == 'n1_fully_masked':          # no key at all: the attention is 0, f = proj.bias, the divergence is exactly 0
        assert torch.equal(l, torch.zeros_like(l))
        b = f.odefunc.diffeq.net.proj.bias.detach().cpu().double()
        assert (y.cpu().double() - (x.double() + 0.7 * b)).abs().max().item() <= 1e-5


def test_zero_rows():
    f = ah.make(2, [12, 8], n_heads=2).to(DEV)
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(torch.zeros(0, 5, 2, device=DEV))
    assert f._last_path == 'kernel' and y.shape == (0, 5, 2) and l.shape == (0, 5, 1)


def test_large_scores_need_the_max_subtraction():
    """Query and key weights scaled until |s| reaches about 60: exp(60) overflows nothing only because the maximum is subtracted."""
    torch.manual_seed(3)
    f = ah.make(2, [8], n_heads=1, T=0.5, biases=True)
    att = f.odefunc.diffeq.net
    x = torch.randn(4, 9, 2)
    with torch.no_grad():
        for _ in range(40):
            u = torch.cat([torch.zeros_like(x[..., :1]), x], -1)
            s = (att.query.net(u) @ att.key.net(u).transpose(-1, -2)) * 8 ** -0.5
            if s.abs().max().item() >= 60:
                break
            att.query.net[0].weight.mul_(1.3)
            att.key.net[0].weight.mul_(1.3)
    assert 60 <= s.abs().max().item() < 200
    _both_ways('large_scores', f, x)


def _kernel(f, x, lat=None, reverse=False):
    kw = {} if lat is None else {'latent': lat.to(DEV)}
    with torch.no_grad():
        y, l = (f.inverse_and_log_det_jacobian if reverse else f.forward_and_log_det_jacobian)(x.to(DEV), **kw)
    assert f._last_path == 'kernel'
    return y.cpu(), l.cpu()


def test_set_independence_is_bitwise_and_position_is_within_the_bound():
    torch.manual_seed(21)
    f = ah.make(2, [12, 8], n_heads=2, latent=2, biases=True)
    x, lat = torch.randn(12, 5, 2), torch.randn(12, 5, 2)
    y64, l64 = ah.solve64(f, x[4], lat[4])                                 # the moved set alone: its own fp64 values and fp32 error
    y32, l32 = ah.solve32(f, x[4], lat[4])
    f = f.to(DEV)
    y, l = _kernel(f, x, lat)
    _check('slot 4 y', y[4], y32, y64)
    _check('slot 4 ldj', l[4], l32, l64)
    x2, lat2 = torch.randn(12, 5, 2) * 3, torch.randn(12, 5, 2)
    x2[4], lat2[4] = x[4], lat[4]
    y2, l2 = _kernel(f, x2, lat2)
    assert torch.equal(y2[4], y[4]) and torch.equal(l2[4], l[4])          # the same slot, other neighbours: bit for bit
    assert not torch.equal(y2[3], y[3])
    perm = torch.tensor([7, 4, 0, 1, 2, 3, 5, 6, 8, 9, 10, 11])           # set 4 moves to slot 1 (another wave offset) ...
    y3, l3 = _kernel(f, x[perm], lat[perm])
    _check('slot 1 y', y3[1], y32, y64)
    _check('slot 1 ldj', l3[1], l32, l64)
    big = torch.cat([x2, x2, x2[:1], x[4:5], x2[:3]]), torch.cat([lat2, lat2, lat2[:1], lat[4:5], lat2[:3]])      # 25 sets fill a pass:
    y4, l4 = _kernel(f, *big)                                              # ... and to the front of pass 1: a second workgroup's FIRST
    # trip (the grid is 2 here; a workgroup's second and later trips round the pass loop: test_gpu_cnf_passes.py)
    _check('second pass y', y4[25], y32, y64)
    _check('second pass ldj', l4[25], l32, l64)


def test_permutation_equivariance():
    torch.manual_seed(22)
    f = ah.make(3, [16], n_heads=4, mask_diagonal=True, biases=True)
    x = torch.randn(3, 37, 3)
    perm = torch.randperm(37)
    y64, l64 = ah.solve64(f, x)
    y32, l32 = ah.solve32(f, x)
    f = f.to(DEV)
    yp, lp = _kernel(f, x[:, perm])
    _check('permuted y', yp, y32[:, perm], y64[:, perm])
    _check('permuted ldj', lp, l32[:, perm], l64[:, perm])


def test_round_trip():
    """inverse(forward(x)) on the kernel within 8 x the fp32 sequence's own round-trip error (grid + fp32; floor 1e-6 * max(1, max |.|))."""
    torch.manual_seed(23)
    f = ah.make(2, [24, 16], n_heads=2, latent=3, step=1 / 16, biases=True)
    x, lat = torch.randn(6, 11, 2), torch.randn(6, 11, 3)
    y32, l32 = ah.solve32(f, x, lat)
    xb32, lb32 = ah.solve32(f, y32, lat, reverse=True)
    e_rt = (xb32 - x).abs().max().item()
    e_ld = (l32 + lb32).abs().max().item()
    f = f.to(DEV)
    y, l = _kernel(f, x, lat)
    xb, lb = _kernel(f, y, lat, reverse=True)
    rt = (xb - x).abs().max().item()
    ld = (l + lb).abs().max().item()
    print(f'round trip {rt:.3e} (fp32 sequence {e_rt:.3e}), ldj + ldj_back {ld:.3e} (fp32 sequence {e_ld:.3e})')
    assert rt <= max(8 * e_rt, 1e-6 * max(1.0, x.abs().max().item()))
    assert ld <= max(8 * e_ld, 1e-6 * max(1.0, l.abs().max().item()))


@pytest.mark.parametrize('hidden,act', [([8], None), ([12, 8], 'Tanh'), ([12, 8], 'LeakyReLU'), ([12, 8], 'ReLU')])
def test_non_finite_sets_stay_alone(hidden, act):
    """One set with a NaN and one with an Inf among finite neighbours of the same workgroup: the poisoned sets come back non-finite in
    every element (the reference's p @ v multiplies every row by the NaN / Inf value), every other set bit for bit as without them.
    Behind a Tanh an Inf becomes a finite +-1 and only the row itself is lost, as in the reference: that configuration carries the NaN
    alone, LeakyReLU takes the Inf through both layers.  ReLU: torch keeps a NaN hidden unit where fmaxf(v, 0) would drop it."""
    torch.manual_seed(24)
    f = ah.make(2, hidden, n_heads=2, act=act, biases=True).to(DEV)
    x = torch.randn(12, 5, 2)
    y, l = _kernel(f, x)
    xp = x.clone()
    xp[3, 2, 0] = float('nan')
    bad = [3]
    if act != 'Tanh':
        xp[7, 0, 1] = float('inf')
        bad.append(7)
    yp, lp = _kernel(f, xp)
    xb, lb = _kernel(f, xp, reverse=True)
    x0, l0 = _kernel(f, x, reverse=True)
    good = [i for i in range(12) if i not in bad]
    for got, clean in ((yp, y), (lp, l), (xb, x0), (lb, l0)):
        assert not torch.isfinite(got[bad]).any()
        assert torch.equal(got[good], clean[good])


def test_forward_inverse_and_no_divergence():
    torch.manual_seed(25)
    f = ah.make(2, [12, 8], n_heads=2, biases=True).to(DEV)
    x = torch.randn(5, 7, 2, device=DEV)
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(x)
        assert torch.equal(f.forward(x), y) and f._last_path == 'kernel'
        assert torch.equal(f.log_det_jacobian(x), l)
        xb, lb = f.inverse_and_log_det_jacobian(y)
        assert torch.equal(f.inverse(y), xb) and f._last_path == 'kernel'
    g = ah.make(2, [12, 8], n_heads=2, divergence='none').to(DEV)
    g.load_state_dict(f.state_dict())
    with torch.no_grad():
        y0, l0 = g.forward_and_log_det_jacobian(x)
    assert g._last_path == 'kernel' and torch.equal(y0, y) and torch.equal(l0, torch.zeros_like(l)) and l0.shape == l.shape
    assert g._num_evals() == 16


class _Sub(st.net.SelfAttention):
    pass


@pytest.mark.parametrize('gate', ['mask', 'graph', 'training', 'heads3', 'three_layers', 'subclass'])
def test_gates_take_the_composition_path(gate):
    torch.manual_seed(26)
    hidden, heads = ([12], 3) if gate == 'heads3' else ([6, 6, 8], 2) if gate == 'three_layers' else ([12, 8], 2)
    f = ah.make(2, hidden, n_heads=heads, T=0.5, biases=True)
    x = torch.randn(3, 4, 2)
    y64, l64 = ah.solve64(f, x)
    y32, l32 = ah.solve32(f, x)
    if gate == 'subclass':
        f.odefunc.diffeq.net.__class__ = _Sub
    f = f.to(DEV)
    xd, kw = x.to(DEV), {}
    if gate == 'mask':
        kw['mask'] = torch.ones(3, 4, 1, device=DEV)
    if gate == 'graph':
        xd.requires_grad_(True)
    if gate == 'training':
        f.train()
        y, l = f.forward_and_log_det_jacobian(xd, **kw)
    elif gate == 'graph':
        y, l = f.forward_and_log_det_jacobian(xd, **kw)
        assert y.requires_grad
    else:
        with torch.no_grad():
            y, l = f.forward_and_log_det_jacobian(xd, **kw)
    assert f._last_path == 'composed'
    _check(f'{gate} y', y.detach(), y32, y64)
    _check(f'{gate} ldj', l.detach(), l32, l64)
    if gate in ('mask', 'graph', 'training', 'subclass'):          # the kernel applies to the same module without the gate
        f.eval()
        f.odefunc.diffeq.net.__class__ = st.net.SelfAttention
        yk, lk = _kernel(f, x)
        _check(f'{gate} kernel y', yk, y32, y64)
        _check(f'{gate} kernel ldj', lk, l32, l64)


def test_in_place_weight_update_changes_the_next_result():
    torch.manual_seed(27)
    f = ah.make(2, [12, 8], n_heads=2, biases=True).to(DEV)
    x = torch.randn(4, 6, 2)
    y, l = _kernel(f, x)
    with torch.no_grad():
        f.odefunc.diffeq.net.value.net[2].weight.mul_(1.5)
        f.odefunc.diffeq.net.proj.bias.add_(0.1)
    y2, l2 = _kernel(f, x)
    assert not torch.equal(y2, y) and not torch.equal(l2, l)
    g = ah.make(2, [12, 8], n_heads=2)
    g.load_state_dict(f.state_dict())
    y64, l64 = ah.solve64(g, x)
    y32, l32 = ah.solve32(g, x)
    _check('updated y', y2, y32, y64)
    _check('updated ldj', l2, l32, l64)


def test_training_through_the_composition_path():
    torch.manual_seed(28)
    f = ah.make(2, [12, 8], n_heads=2, mask_diagonal=True, biases=True).to(DEV).train()
    x = torch.randn(3, 4, 2, device=DEV)
    y, ldj = f.forward_and_log_det_jacobian(x)
    assert f._last_path == 'composed'
    (-ldj.mean() + y.square().mean()).backward()
    for n, p in f.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert sum(p.grad.abs().sum().item() for p in f.parameters()) > 0
