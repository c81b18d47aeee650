"""GPU: ContinuousTransform trained on sx_cnf_train_fwd / sx_cnf_train_bwd (divergence='approximate', training mode).

The truth is the fp64 CPU restatement of the solve with the Hutchinson estimate for the noise the call drew (cnftrainhelp.truth:
reverse mode twice).  The reference error e_ref is the composition path on the GPU in fp32 with the same module and seed -- a mask
of ones forces it, DiffeqMLP ignores the mask.  Per tensor the bound is cnfhelp.bound: 8 e_ref, floor 1e-6 max(1, max |truth|); for
parameter gradients the floor is 8 K 2^-23 max(1, max |truth|), K = steps x stages.

The kernels cover hidden layers of <= 32 units (DESIGN.md "CNF training"): the nets (32, [33]), (6, [40, 24], 2) and (5, [64, 64], 58)
of the gradient cases are outside that and pin the composition path; (32, [32]), (6, [32, 24], 2) and (5, [32, 32], 58) reach the
same edges -- a full state tile, unequal widths, two latent tiles -- inside it."""
import pytest
import torch

import stribor_amd as st

import cnfhelp as ch
import cnftrainhelp as th
import passhelp as ph

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

NETS = [(3, [5], 0), (32, [33], 0), (6, [40, 24], 2), (5, [64, 64], 58), (32, [32], 0), (6, [32, 24], 2), (5, [32, 32], 58)]


def _covered(hidden):
    return max(hidden) <= 32


def _both(f, x, lat, reverse, tag, expect='kernel'):
    got = th.run(f, x, lat, reverse)
    assert got['path'] == expect, (tag, got['path'])
    ref = th.run(f, x, lat, reverse, mask=torch.ones(*x.shape[:-1], 1, device=x.device))
    assert ref['path'] == 'composed'
    assert torch.equal(got['e'], ref['e']), tag
    want = th.truth(f, x, got['e'], lat, reverse)
    n_evals = (len(ch.grid64(0.0, f.T, f.solver_options['step_size'])) - 1) * th.STAGES[f.solver]
    assert got['evals'] == n_evals
    return th.check(tag, got, ref, want, n_evals)


@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('solver', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('net', NETS, ids=lambda n: f'{n[0]}-{"x".join(map(str, n[1]))}-{n[2]}')
def test_gradients_and_values(net, solver, reverse):
    dim, hidden, latent = net
    f = th.make(dim, hidden, latent, solver=solver, seed=dim + latent).to(DEV)
    g = torch.Generator().manual_seed(5)
    for n in (1, 33, 130):                         # (130 rows: two workgroups, more than one partial per gradient)
        x = torch.randn(n, dim, generator=g).to(DEV)
        lat = torch.randn(n, latent, generator=g).to(DEV) if latent else None
        _both(f, x, lat, reverse, f'{net} {solver} reverse={reverse} n={n}', 'kernel' if _covered(hidden) else 'composed')


@pytest.mark.parametrize('act', th.ACTIVATIONS)
def test_every_activation(act):
    f = th.make(6, [24, 24], 2, activation=act, seed=3).to(DEV)
    g = torch.Generator().manual_seed(6)
    x, lat = torch.randn(33, 6, generator=g).to(DEV), torch.randn(33, 2, generator=g).to(DEV)
    _both(f, x, lat, True, act)


def test_rademacher_noise():
    f = th.make(6, [24], 2, rademacher=True, seed=4).to(DEV)
    g = torch.Generator().manual_seed(7)
    x, lat = torch.randn(33, 6, generator=g).to(DEV), torch.randn(33, 2, generator=g).to(DEV)
    _both(f, x, lat, True, 'rademacher')
    assert set(f.odefunc._e.unique().tolist()) <= {-1.0, 1.0}


@pytest.mark.parametrize('solver', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('net', [(3, [5], 0), (6, [32, 24], 2), (5, [32, 32], 58)])
def test_forward_value_is_the_eval_kernels(net, solver):
    dim, hidden, latent = net
    f = th.make(dim, hidden, latent, solver=solver, seed=8).to(DEV)
    x = torch.randn(130, dim, device=DEV)
    lat = torch.randn(130, latent, device=DEV) if latent else None
    y = f(x, latent=lat)
    assert f._last_path == 'kernel' and y.requires_grad
    f.eval()
    with torch.no_grad():
        y_eval = f(x, latent=lat)
    assert f._last_path == 'kernel'
    assert torch.equal(y.detach(), y_eval)


def test_noise_and_rng_stream_match_the_composition_path():
    f = th.make(4, [16], seed=9).to(DEV)
    x = torch.randn(3, 7, 4, device=DEV)
    ones = torch.ones(3, 7, 1, device=DEV)
    for rademacher in (False, True):
        f.odefunc.rademacher = rademacher
        states = []
        for mask in (None, ones):
            torch.manual_seed(21)
            f.forward_and_log_det_jacobian(x, mask=mask)
            states.append((f._last_path, f.odefunc._e.clone(), torch.get_rng_state(), torch.cuda.get_rng_state(0)))
        (pa, ea, ca, ga), (pb, eb, cb, gb) = states
        assert (pa, pb) == ('kernel', 'composed')
        assert ea.shape == x.shape and torch.equal(ea, eb)
        assert torch.equal(ca, cb) and torch.equal(ga, gb)


def test_routing():
    dim = 3
    x = torch.randn(9, dim, device=DEV)
    f = th.make(dim, [16], solver='rk4', step=0.25, T=0.7).to(DEV)
    torch.manual_seed(1)
    y, l = f.forward_and_log_det_jacobian(x)
    assert f._last_path == 'kernel' and f._num_evals() == 3 * 4 and y.requires_grad and l.requires_grad and l.shape == (9, 1)
    torch.manual_seed(1)
    with torch.no_grad():
        y0, l0 = f.forward_and_log_det_jacobian(x)
    assert f._last_path == 'kernel' and not y0.requires_grad
    assert torch.equal(y0, y.detach()) and torch.equal(l0, l.detach())
    for g, why in ((th.make(dim, [16], divergence='compute'), 'compute'), (th.make(dim, [16]).eval(), 'eval'),
                   (th.make(dim, [65]), 'hidden 65'), (th.make(dim, [16], set_data=True), 'set_data')):
        g = g.to(DEV)
        g.forward_and_log_det_jacobian(x.reshape(1, 9, dim) if why == 'set_data' else x)
        assert g._last_path == 'composed', why


def test_frozen_parameters_and_input_gradient():
    f = th.make(4, [16], 2, seed=12).to(DEV)
    frozen = th.params(f)[0:2]
    for p in frozen:
        p.requires_grad_(False)
    x, lat = torch.randn(33, 4, device=DEV), torch.randn(33, 2, device=DEV)
    got = th.run(f, x, lat, True)
    assert got['path'] == 'kernel'
    assert all(p.grad is None for p in frozen) and all(p.grad is not None for p in th.params(f)[2:])
    # x alone, every weight frozen
    for p in f.parameters():
        p.requires_grad_(False)
    got = th.run(f, x, lat, True)
    assert got['path'] == 'kernel' and all(p.grad is None for p in f.parameters())
    ref = th.run(f, x, lat, True, mask=torch.ones(33, 1, device=DEV))
    want = th.truth(f, x, got['e'], lat, True)
    for k in ('gx', 'glat'):
        tol, e_ref = ch.bound(ref[k].cpu(), want[k])
        err = (got[k].cpu().double() - want[k]).abs().max().item()
        print(f'frozen {k}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e}')
        assert err <= tol


def test_second_differentiation_raises():
    f = th.make(3, [8], seed=13).to(DEV)
    x = torch.randn(5, 3, device=DEV, requires_grad=True)
    y, l = f.forward_and_log_det_jacobian(x)
    assert f._last_path == 'kernel'
    (gx,) = torch.autograd.grad(th.loss_of(y, l), x, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable|differentiate twice'):
        gx.sum().backward()


def test_backward_is_deterministic():
    f = th.make(5, [32, 32], 58, seed=14).to(DEV)
    x, lat = torch.randn(130, 5, device=DEV), torch.randn(130, 58, device=DEV)
    a, b = th.run(f, x, lat, True), th.run(f, x, lat, True)
    assert a['path'] == 'kernel'
    for k in ('y', 'ldj', 'gx', 'glat'):
        assert torch.equal(a[k], b[k]), k
    for i, (p, q) in enumerate(zip(a['params'], b['params'])):
        assert torch.equal(p, q), i


def _sum_loss(y, ldj):
    return (0.5 * (y * y).sum(-1) - ldj.reshape(y.shape[:-1])).sum()


def test_second_and_later_passes_per_workgroup(monkeypatch):
    """Every workgroup of the backward takes a second trip round its pass loop with its accumulators live (passhelp's batch): the rows
    tile a short period, so y, ldj and gx repeat the period's bit for bit and every parameter gradient of a SUM loss is copies x the
    period's plus the remainder rows' share."""
    f = th.make(2, [8], solver='euler', step=0.4, T=0.7, seed=15).to(DEV)          # two steps
    n = ph.big_rows(DEV)
    ph.assert_multi_pass(n, 1, DEV)
    g = ph.generator('cnf_train_passes')
    small = torch.randn(ph.ROW_PERIOD, 2, generator=g).to(DEV)
    noise = torch.randn(ph.ROW_PERIOD, 2, generator=g).to(DEV)
    copies, rest = divmod(n, ph.ROW_PERIOD)
    # the same noise row for every copy of a row: the noise is the module's to draw, so hand it the tiled one
    monkeypatch.setattr(f, '_draw_noise', lambda x: setattr(f.odefunc, '_e', ph.tile(noise, x.shape[0])) or f.odefunc._e)
    one = th.run(f, small, loss=_sum_loss)
    ph.poison_outputs(monkeypatch, DEV)
    big = th.run(f, ph.tile(small, n), loss=_sum_loss)
    assert one['path'] == big['path'] == 'kernel'
    for k in ('y', 'ldj', 'gx'):
        ph.assert_tiled(k, big[k], one[k])
    want = th.truth(f, small, noise, loss=_sum_loss)
    tail = th.truth(f, small[:rest], noise[:rest], loss=_sum_loss)
    # the composition path on the period with the same noise: its first evaluation keeps an _e that is already there
    monkeypatch.setattr(f.odefunc, 'before_odeint', lambda e=None: setattr(f.odefunc, '_e', noise))
    ref = th.run(f, small, loss=_sum_loss, mask=torch.ones(ph.ROW_PERIOD, 1, device=DEV))
    assert ref['path'] == 'composed' and torch.equal(ref['e'], noise)
    worst = 0.0
    for i, (a, r, w, t) in enumerate(zip(big['params'], ref['params'], want['params'], tail['params'])):
        total = copies * w + t
        e_ref = (r.cpu().double() - w).abs().max().item()
        tol = max(8 * (copies + 1) * e_ref, 8 * 2 * 2.0 ** -23 * max(1.0, total.abs().max().item()))
        err = (a.cpu().double() - total).abs().max().item()
        worst = max(worst, err / tol)
        print(f'param {i}: err {err:.3e} bound {tol:.3e} of |total| {total.abs().max().item():.3e}')
        assert err <= tol, (i, err, tol)
    print(f'multi-pass: {n} rows, worst error / bound {worst:.3f}')


def test_unaligned_views_reproduce_the_aligned_results():
    f = th.make(5, [16], 3, seed=16).to(DEV)
    lib_fwd, lib_bwd = 'sx_cnf_train_fwd', 'sx_cnf_train_bwd'
    n, dim, L = 37, 5, 3
    x, e, lat, gy = (torch.randn(n, w, device=DEV) for w in (dim, dim, L, dim))
    gl = torch.randn(n, device=DEV)
    name, step, grid = f._grid(True)

    def offset(t):
        buf = torch.empty(t.numel() + 1, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 8 == 4 or v.data_ptr() % 16 != 0
        return v

    def call(x, e, lat, gy):
        ckpt = torch.empty(len(grid) - 1, n, dim, device=DEV)
        y, ldj = f._train_forward(x, lat, e, name, step, grid, ckpt)
        y2, _ = st.flows.cnf._CNFTrain.apply(f, name, step, grid, x.requires_grad_(True), lat.requires_grad_(True), e, *th.params(f))
        gx, glat, *gp = torch.autograd.grad(y2, [x, lat] + th.params(f), gy)
        return [y, ldj, gx, glat] + gp

    want = call(x.clone(), e.clone(), lat.clone(), gy.clone())
    got = call(offset(x), offset(e), offset(lat), offset(gy))
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    assert lib_fwd in st._hip.EXPORTS and lib_bwd in st._hip.EXPORTS


def test_in_a_normalizing_flow(monkeypatch):
    """log_prob runs the layers in inverse order: x -> CNF (reverse) -> coupling -> base.  One backward() takes the kernel path in the
    CNF layer; the coupling's and the CNF's parameters receive the gradients of the fp64 restatement (the coupling by the oracle)."""
    import numpy as np
    from oracle import stribor_oracle as orc
    from stribor_amd.util import flowdesc as fd
    dim = 2
    torch.manual_seed(17)
    coupling = st.Coupling(st.Affine(dim, latent_net=st.net.MLP(dim, [13], 2 * dim)), mask='ordered_1')
    cnf = th.make(dim, [13], solver='rk4', step=0.25, T=1.0, seed=18)
    flow = st.NormalizingFlow(st.UnitNormal(dim), [coupling, cnf]).to(DEV).train()
    x = torch.randn(50, dim, device=DEV)
    names = [n for n, _ in coupling.named_parameters()]

    def grads():
        flow.zero_grad(set_to_none=True)
        torch.manual_seed(19)
        (-flow.log_prob(x).mean()).backward()
        return [p.grad.detach().clone() for p in list(coupling.parameters()) + th.params(cnf)], cnf._last_path, cnf.odefunc._e
    got, path, e = grads()
    assert path == 'kernel' and cnf._num_evals() == 16
    with monkeypatch.context() as m:
        m.setattr(cnf, '_train_kernel_net', lambda *a: None)
        ref, path, e_ref_noise = grads()
    assert path == 'composed' and torch.equal(e, e_ref_noise)
    state = {k: v.detach().cpu().double().requires_grad_(True) for k, v in flow.state_dict().items() if k.startswith('transforms.0.')}
    spec = fd.transform_spec({'kind': 'coupling_affine', 'dim': dim, 'hidden': [13], 'mask': 'ordered_1'}, state, 'transforms.0.')

    def loss(z, l):
        y, lc = orc.transform_inverse_and_ldj(spec, z)
        return (0.5 * (y * y).sum(-1) + 0.5 * dim * np.log(2 * np.pi) - l - lc.reshape(l.shape)).mean()
    t = th.truth(cnf, x, e, reverse=True, loss=loss)
    want = list(torch.autograd.grad(loss(t['y'], t['ldj'].squeeze(-1)), [state['transforms.0.' + n] for n in names])) + t['params']
    worst = 0.0
    for i, (a, r, w) in enumerate(zip(got, ref, want)):
        e_ref = (r.cpu().double() - w).abs().max().item()
        tol = max(8 * e_ref, 8 * 16 * 2.0 ** -23 * max(1.0, w.abs().max().item()))
        err = (a.cpu().double() - w).abs().max().item()
        worst = max(worst, err / tol)
        assert err <= tol, (i, err, e_ref, tol)
    print(f'in a flow: worst error / bound {worst:.3f}')
