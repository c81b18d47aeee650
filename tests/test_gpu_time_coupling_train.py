"""GPU: training ContinuousAffineCoupling / NeuralFlow on sx_time_coupling_bwd -- gradients of single layers and of whole flows against
fp64 autograd of the oracle, the values and bits of a graph-building call, the kernel's second and later passes, the layers outside
the coverage, and accumulation into existing gradients.

Tolerances are cnfhelp.bound's: the composed path (`_run_composed`: torch ops around AffineCouplingOp, the same build, the same inputs)
has its own fp32 error against the fp64 oracle gradient; the kernel path must stay within 8 x that (floor 1e-6 * max(1, max |truth|)).
Nothing is compared against the code under test."""
import pytest
import torch

import stribor_amd as st
from oracle import stribor_oracle as orc
from stribor_amd.flows.coupling import ContinuousAffineCoupling

import cnfhelp as ch
import passhelp as ph
import timecouplinghelp as th

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (D, H, L, mask): the issue's shapes, then one shape per remaining instantiation of the kernel (input tiles, hidden tiles, live tiles)
SHAPES = [(4, 16, 0, 'ordered_left_half'), (4, 16, 3, 'parity_odd'), (33, 40, 5, 'random_half'), (64, 64, 0, 'ordered_right_half'),
          (1, 8, 2, 'none')]
EXTRA = [(64, 64, 0, 'none'), (40, 20, 0, 'none'), (24, 16, 30, 'parity_odd'), (24, 40, 30, 'parity_even')]
ROWS = (1, 33, 129, 300)
KINDS = ('identity', 'linear', 'tanh', 'log')
MODE_NAMES = ('forward', 'inverse', 'forward_and_log_det_jacobian', 'inverse_and_log_det_jacobian')


def _check(tag, got, ref, truth):
    if truth is None:
        assert got is None, tag
        return
    tol, e_ref = ch.bound(ref.detach().cpu(), truth)
    err = (got.detach().cpu().double() - truth).abs().max().item()
    print(f'{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e}')
    assert got.shape == truth.shape, tag
    assert err <= tol, (tag, err, e_ref, tol)


def _compare(f, mode, data):
    """-> the oracle's fp64 gradients, the composed path's and those of an ordinary call of `f` on `data`."""
    want = th.truth(f, mode, *data)
    ref, _, _ = th.run(f, mode, *data, composed=True)
    f._last_path = None
    got, _, _ = th.run(f, mode, *data)
    return want, ref, got


def _single(monkeypatch, shape, n, kind, half_is_dim, concat, mode, act='Tanh', seed=0):
    D, H, L, mask = shape
    f = th.make_layer(D, H, L, kind, D if half_is_dim else 1, concat, act, mask, seed=seed)
    th.oracle_masks(monkeypatch, [f], D)
    data = th.inputs(n, D, L, seed=seed + 17)
    f = f.to(DEV)
    want, ref, got = _compare(f, mode, data)
    assert f._last_path == 'kernel'
    for k in want:
        _check(f'{shape} n={n} {kind} {mode} {k}', got[k], ref[k], want[k])


# every (shape, rows) pair; the time kind, its half-width, the time column and the method rotate through their values so that each
# occurs with every shape and every row count
@pytest.mark.parametrize('si,ni', [(s, n) for s in range(len(SHAPES)) for n in range(len(ROWS))])
def test_single_layer_gradients(monkeypatch, si, ni):
    i = si * len(ROWS) + ni
    for j in range(2):                  # two of the rotating combinations per pair
        k = 2 * i + j
        _single(monkeypatch, SHAPES[si], ROWS[ni], KINDS[(si + ni + j) % 4], (k // 2) % 2 == 0, (k // 3) % 2 == 0, MODE_NAMES[(ni + 2 * j + si) % 4],
                seed=k)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('half_is_dim', [True, False])
@pytest.mark.parametrize('concat', [True, False])
@pytest.mark.parametrize('mode', MODE_NAMES)
def test_every_time_net_direction_and_log_det(monkeypatch, kind, half_is_dim, concat, mode):
    """The full product of time kind x half-width x time column x method, on one shape with a latent and a ragged row count."""
    _single(monkeypatch, SHAPES[1], 33, kind, half_is_dim, concat, mode, seed=5)


@pytest.mark.parametrize('shape', EXTRA, ids=str)
def test_the_other_tile_counts(monkeypatch, shape):
    _single(monkeypatch, shape, 129, 'tanh', True, True, 'inverse_and_log_det_jacobian', seed=9)
    _single(monkeypatch, shape, 33, 'log', False, True, 'forward_and_log_det_jacobian', seed=10)


@pytest.mark.parametrize('act', th.ACTIVATIONS)
def test_the_seven_activations(monkeypatch, act):
    _single(monkeypatch, SHAPES[1], 33, 'tanh', True, True, 'forward_and_log_det_jacobian', act=act, seed=21)


def test_only_x_requires_grad_touches_no_partial(monkeypatch):
    """Every parameter frozen: one launch, no partial buffer, no parameter gradient -- and gx as with them."""
    D, H, L, mask = SHAPES[1]
    f = th.make_layer(D, H, L, 'tanh', D, True, 'Tanh', mask, seed=2)
    th.oracle_masks(monkeypatch, [f], D)
    data = th.inputs(129, D, L, seed=4)
    want = th.truth(f, 'forward_and_log_det_jacobian', *data)
    f = f.to(DEV)
    for p in f.parameters():
        p.requires_grad_(False)
    calls = {'partial_floats': 0, 'partial': []}
    lib = st._hip.lib()
    size_fn, call = lib.sx_time_coupling_bwd_partial_floats, st._hip.call

    def counting(*a):
        calls['partial_floats'] += 1
        return size_fn(*a)

    def spying(name, like, *args):
        if name == 'sx_time_coupling_bwd':
            calls['partial'].append(args[9])
        return call(name, like, *args)
    monkeypatch.setattr(lib, 'sx_time_coupling_bwd_partial_floats', counting)
    monkeypatch.setattr(st._hip, 'call', spying)
    needs = (True, False, False)
    ref, _, _ = th.run(f, 'forward_and_log_det_jacobian', *data, composed=True, needs=needs)
    got, _, _ = th.run(f, 'forward_and_log_det_jacobian', *data, needs=needs)
    assert f._last_path == 'kernel'
    assert calls == {'partial_floats': 0, 'partial': [None]}
    assert all(p.grad is None for p in f.parameters()) and got['t'] is None and got['latent'] is None
    _check('x only', got['x'], ref['x'], want['x'])


@pytest.mark.parametrize('mode', MODE_NAMES)
def test_values_are_the_no_grad_call_and_two_backwards_give_the_same_bits(monkeypatch, mode):
    D, H, L, mask = SHAPES[2]
    f = th.make_layer(D, H, L, 'tanh', D, True, 'Tanh', mask, seed=6)
    th.oracle_masks(monkeypatch, [f], D)                    # (pins the 'random_half' draw)
    f = f.to(DEV)
    data = th.inputs(300, D, L, seed=8)
    g1, y1, l1 = th.run(f, mode, *data)
    g2, y2, l2 = th.run(f, mode, *data)
    assert f._last_path == 'kernel'
    x, t, lat = (None if v is None else v.to(DEV) for v in data[:3])
    with torch.no_grad():
        out = getattr(f, mode)(x, t, latent=lat)
    y0, l0 = out if isinstance(out, tuple) else (out, None)
    assert torch.equal(y1, y0) and torch.equal(y2, y0)
    assert l0 is None or (torch.equal(l1, l0) and torch.equal(l2, l0))
    for k in g1:
        assert (g1[k] is None and g2[k] is None) or torch.equal(g1[k], g2[k]), k


def _flow(monkeypatch, with_t0, L):
    D, n = 4, 80
    torch.manual_seed(61)
    layers = [th.make_layer(D, 16, L, kind, None, True, 'Tanh', mask, seed=40 + i)
              for i, (mask, kind) in enumerate((('ordered_left_half', 'linear'), ('ordered_right_half', 'tanh'), ('parity_odd', 'log')))]
    nf = st.NeuralFlow(layers)
    th.oracle_masks(monkeypatch, layers, D)
    x, t, lat, target, _ = th.inputs(n, D, L, seed=3)
    t0 = torch.rand(n, 1, generator=torch.Generator().manual_seed(9)) if with_t0 else None
    leaves = th.leaves_of(nf)
    spec = [th.layer_spec(f, leaves, f'transforms.{i}.') for i, f in enumerate(layers)]
    xin = x.double().clone().requires_grad_(True)
    want = ((orc.neural_flow_forward(spec, xin, t.double(), None if t0 is None else t0.double(), None if lat is None else lat.double())
             - target.double()) ** 2).mean()
    want.backward()
    nf = nf.to(DEV)
    kw = {} if lat is None else {'latent': lat.to(DEV)}

    def step():
        nf.zero_grad(set_to_none=True)
        xg = x.to(DEV).requires_grad_(True)
        out = nf(xg, t=t.to(DEV), t0=None if t0 is None else t0.to(DEV), **kw)
        ((out - target.to(DEV)) ** 2).mean().backward()
        return xg.grad, {k: p.grad.clone() for k, p in nf.named_parameters()}
    with monkeypatch.context() as mp:                      # the composed path of every layer: the planner declines
        mp.setattr(ContinuousAffineCoupling, '_train_plan', lambda self, *a: None)
        ref_x, ref_p = step()
        assert all(f._last_path == 'composed' for f in nf.transforms)
    got_x, got_p = step()
    assert all(f._last_path == 'kernel' for f in nf.transforms)
    _check('flow gx', got_x, ref_x, xin.grad)
    for k, v in leaves.items():
        _check(f'flow {k}', got_p[k], ref_p[k], v.grad)


def test_neural_flow_trains_on_the_kernel(monkeypatch):
    _flow(monkeypatch, False, 0)


def test_neural_flow_with_t0_and_latent_trains_on_the_kernel(monkeypatch):
    _flow(monkeypatch, True, 3)


@pytest.mark.parametrize('mode', ['forward_and_log_det_jacobian', 'inverse_and_log_det_jacobian'])
def test_second_and_later_passes(monkeypatch, mode):
    """A batch tiled from a 77-row period, large enough that every workgroup takes its second and later trips round the pass loop: gx is
    the period's row for row, and the parameter gradients are the period's fp64 gradients with each row weighted by how often it occurs.
    Outputs and partials start as NaN, so a word never written shows."""
    D, H, L, mask = SHAPES[1]
    f = th.make_layer(D, H, L, 'tanh', D, True, 'Tanh', mask, seed=12)
    th.oracle_masks(monkeypatch, [f], D)
    n = ph.big_rows(DEV)
    ph.assert_multi_pass(n, 1, DEV)
    period = th.inputs(ph.ROW_PERIOD, D, L, seed=13)
    counts = torch.bincount(torch.arange(n) % ph.ROW_PERIOD, minlength=ph.ROW_PERIOD).double().reshape(-1, 1)
    want = th.truth(f, mode, *period, weight=counts)
    f = f.to(DEV)
    small, _, _ = th.run(f, mode, *period)
    big_data = tuple(ph.tile(v, n) for v in period)
    ref, _, _ = th.run(f, mode, *big_data, composed=True)
    ph.poison_outputs(monkeypatch, DEV)
    got, y, ldj = th.run(f, mode, *big_data)
    assert f._last_path == 'kernel'
    for k in ('x', 't', 'latent'):
        ph.assert_tiled(k, got[k].reshape(n, -1), small[k].reshape(ph.ROW_PERIOD, -1))
    for k, p in f.named_parameters():
        _check(f'passes {k}', got[k], ref[k], want[k])


OUTSIDE = {'H-65': dict(D=4, H=65, L=0), 'two-hidden': dict(D=4, H=16, L=0, hidden=[16, 12]), 'SiLU': dict(D=4, H=16, L=0, act='SiLU'),
           'fourier': dict(D=4, H=16, L=0, kind='fourier'), 'D-65': dict(D=65, H=16, L=0)}


@pytest.mark.parametrize('which', sorted(OUTSIDE))
def test_outside_the_coverage_composes(monkeypatch, which):
    kw = dict(OUTSIDE[which])
    if kw.get('kind') == 'fourier':
        kw['kind'] = st.net.TimeFourier(2 * kw['D'], 5)
    f = th.make_layer(**kw)
    D, L = kw['D'], kw['L']
    th.oracle_masks(monkeypatch, [f], D)
    data = th.inputs(129, D, L, seed=31)
    f = f.to(DEV)
    want, ref, got = _compare(f, 'forward_and_log_det_jacobian', data)
    assert f._last_path == 'composed'
    for k in want:
        _check(f'{which} {k}', got[k], ref[k], want[k])


def test_zero_grad_then_a_second_step_accumulates_correctly():
    D, H, L, mask = SHAPES[1]
    f = th.make_layer(D, H, L, 'log', 1, True, 'Tanh', mask, seed=14).to(DEV)
    x, t, lat, wy, wl = (v.to(DEV) for v in th.inputs(129, D, L, seed=15))

    def backward():
        y, ldj = f.forward_and_log_det_jacobian(x, t, latent=lat)
        th.loss_of(y, ldj, wy, wl, True).backward()
    backward()
    assert f._last_path == 'kernel'
    first = {k: p.grad.clone() for k, p in f.named_parameters()}
    backward()                                              # into the existing .grad: exactly twice the first
    for k, p in f.named_parameters():
        assert torch.equal(p.grad, first[k] + first[k]), k
    f.zero_grad()
    backward()
    for k, p in f.named_parameters():
        assert torch.equal(p.grad, first[k]), k


def test_a_parameter_changed_in_place_before_backward_is_an_error():
    """An optimizer step between two backwards of a retained graph: the backward recomputes the conditioner from the weights, so
    autograd's version check must refuse it (as it does on the composed path), not return gradients of the new weights."""
    D, H, L, mask = SHAPES[1]
    f = th.make_layer(D, H, L, 'tanh', D, True, 'Tanh', mask, seed=16).to(DEV)
    x, t, lat, wy, wl = (v.to(DEV) for v in th.inputs(33, D, L, seed=18))
    opt = torch.optim.SGD(f.parameters(), lr=1e-2)
    y, ldj = f.forward_and_log_det_jacobian(x, t, latent=lat)
    assert f._last_path == 'kernel'
    th.loss_of(y, ldj, wy, wl, True).backward(retain_graph=True)
    opt.step()
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        th.loss_of(y, ldj, wy, wl, True).backward()
