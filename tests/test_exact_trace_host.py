"""CPU: the exact-trace nets (MADE, DiffeqZeroTraceMLP, DiffeqExactTrace(MLP), FuncAndDiagJac, flatten_params) against fixture F17,
their masks, their gradients and the closed-form tangent the kernel evaluates."""
import inspect
import itertools

import numpy as np
import pytest
import torch

import stribor_amd as st
from stribor_amd.net import diffeq_exact_trace as xt

import cnfhelp as ch
import exacthelp as eh


def _signature(fn):
    return {k: (None if p.default is inspect.Parameter.empty else repr(p.default)) for k, p in inspect.signature(fn).parameters.items()
            if k != 'self'}


def test_constructor_signatures():
    want = eh.golden().meta['signatures']
    for name in ('MADE', 'DiffeqZeroTraceMLP', 'DiffeqExactTrace', 'DiffeqExactTraceMLP'):
        assert _signature(getattr(st.net, name).__init__) == want[name], name


@pytest.mark.parametrize('case', eh.case_names())
def test_state_keys_seeded_weights_and_strict_load(case):
    g = eh.golden()
    m = g.meta['cases'][case]
    f = eh.construct(m)
    state = f.state_dict()
    assert list(state) == m['keys']
    for k, h in m['state_sha256'].items():
        assert ch.sha(state[k]) == h, f'{case}: {k} differs from the reference\'s draw'
    f.load_state_dict(g.state(case), strict=True)
    for k, v in f.state_dict().items():
        assert torch.equal(v, g.t(f'{case}/state/{k}'))
    assert st.util.flatten_params(f.odefunc.diffeq).numel() == sum(p.numel() for p in f.parameters())


@pytest.mark.parametrize('natural,reverse,per_dim,in_dim', list(itertools.product((True, False), (False, True), (False, True), (1, 2, 10))))
def test_made_zero_trace(natural, reverse, per_dim, in_dim):
    torch.manual_seed(in_dim)
    k = 8
    net = st.net.MADE(in_dim, [19, 23], k * in_dim, natural_ordering=natural, reverse_ordering=reverse, return_per_dim=per_dim).double()
    x = torch.randn(in_dim, dtype=torch.float64)
    y = net(x)
    assert y.shape == ((in_dim, k) if per_dim else (k * in_dim,))
    J = torch.autograd.functional.jacobian(lambda v: net(v).reshape(in_dim, k), x)          # [in_dim, k, in_dim]
    for i in range(in_dim):
        assert torch.all(J[i, :, i] == 0)


def test_natural_orderings_are_triangular():
    torch.manual_seed(0)
    D, k = 6, 3
    net = st.net.DiffeqZeroTraceMLP(D, [17, 11], k * D).double()
    x = torch.randn(D, dtype=torch.float64)
    J1 = torch.autograd.functional.jacobian(lambda v: net.net1(v), x)                        # [D, k, D]
    J2 = torch.autograd.functional.jacobian(lambda v: net.net2(v), x)
    for i in range(D):
        assert torch.all(J1[i, :, i:] == 0) and torch.all(J2[i, :, :i + 1] == 0)
    y, jac = net(torch.zeros(1), x)
    assert torch.all(jac == 0) and jac.shape == x.shape and y.shape == (k * D,)
    J = torch.autograd.functional.jacobian(lambda v: net(torch.zeros(1), v)[0].reshape(D, k), x)
    assert all(torch.all(J[i, :, i] == 0) for i in range(D))
    assert J.abs().sum() > 0


def test_update_masks_redraws_only_with_several_masks():
    torch.manual_seed(0)
    one = st.net.MADE(5, [40, 40], 5)
    before = [l.mask.clone() for l in one.masked_linears()]
    one.update_masks()
    assert all(torch.equal(a, l.mask) for a, l in zip(before, one.masked_linears()))
    two = st.net.MADE(5, [40, 40], 10, num_masks=2)
    versions = [l.mask._version for l in two.masked_linears()]
    two.update_masks()
    assert all(l.mask._version > v for l, v in zip(two.masked_linears(), versions))
    for l in two.masked_linears():
        assert l.mask.shape == l.weight.shape and set(l.mask.unique().tolist()) <= {0.0, 1.0}
    x = torch.randn(5, dtype=torch.float64)
    J = torch.autograd.functional.jacobian(lambda v: two.double()(v).reshape(5, 2), x)          # (dimension-major)
    assert all(torch.all(J[i, :, i] == 0) for i in range(5))


@pytest.mark.parametrize('case', eh.case_names())
def test_bare_net_against_fixture(case):
    g = eh.golden()
    f, x, lat, m = eh.build_case(case)
    net = f.odefunc.diffeq
    dy, jac = net(torch.tensor([0.3]), x, latent=lat)
    dy64, jac64 = eh.diag64(eh.net64(net, lat), float(np.float32(0.3)), x)          # (the fixture's t is the fp32 value)
    for name, got, ref, truth in (('dy', dy, g.t(f'{case}/bare_dy'), dy64), ('jac', jac, g.t(f'{case}/bare_jac'), jac64)):
        tol, e_ref = ch.bound(ref, truth)
        err = (got.double() - truth).abs().max().item()
        print(f'{case} {name}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e}')
        assert got.shape == ref.shape
        assert err <= tol, (case, name, err, e_ref, tol)
    assert net.__class__(m['shape'][-1], m['hidden'], m['shape'][-1], m['d_h'], latent_dim=m['latent'], return_log_det_jac=False)(
        torch.tensor([0.3]), x, latent=lat).shape == x.shape


@pytest.mark.parametrize('latent_dim', [0, 3])
@pytest.mark.parametrize('hidden', [[], [8, 4]])
def test_func_and_diag_jac_gradients(latent_dim, hidden):
    """Parameter (and input) gradients of y.mean() through FuncAndDiagJac equal those of the un-detached composition."""
    torch.manual_seed(7)
    D, d_h = 3, 2
    net = st.net.DiffeqExactTraceMLP(D, hidden, D, d_h, latent_dim=latent_dim).double()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.1 * torch.randn_like(p))                 # (the dimwise net's last bias starts at zero)
    x = torch.randn(5, D, dtype=torch.float64, requires_grad=True)
    lat = torch.randn(5, latent_dim, dtype=torch.float64, requires_grad=True) if latent_dim else None
    t = torch.tensor([0.4], dtype=torch.float64)
    y, jac = net(t, x, latent=lat)
    (y.mean() + (jac * jac).mean()).backward()
    got = {k: p.grad.clone() for k, p in net.named_parameters()}
    gx, gl = x.grad.clone(), (None if lat is None else lat.grad.clone())
    # the un-detached composition over substitute leaves
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    leaves = {k: sd[k].requires_grad_(True) for k, _ in net.named_parameters()}
    x2 = x.detach().clone().requires_grad_(True)
    lat2 = None if lat is None else lat.detach().clone().requires_grad_(True)
    y2 = eh.apply64(net, sd, 0.4, x2, lat2)
    jac2 = torch.stack([torch.autograd.grad(y2[..., i].sum(), x2, create_graph=True)[0][..., i] for i in range(D)], -1)
    torch.testing.assert_close(y.detach(), y2.detach(), rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(jac.detach(), jac2.detach(), rtol=1e-10, atol=1e-12)
    (y2.mean() + (jac2 * jac2).mean()).backward()
    for k, leaf in leaves.items():
        want = torch.zeros_like(leaf) if leaf.grad is None else leaf.grad
        torch.testing.assert_close(got[k], want, rtol=1e-10, atol=1e-12, msg=lambda s: f'{k}: {s}')
    torch.testing.assert_close(gx, x2.grad, rtol=1e-10, atol=1e-12)
    if lat is not None:
        torch.testing.assert_close(gl, lat2.grad, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('hidden', [[24], [40, 24]])
@pytest.mark.parametrize('act', ['Tanh', 'Softplus', 'ELU'])
def test_closed_form_tangent(hidden, act):
    torch.manual_seed(11)
    D, d_h, L = 5, 3, 2
    net = st.net.DiffeqExactTraceMLP(D, hidden, D, d_h, latent_dim=L)
    if act != 'Tanh':                                         # the constructors take no activation: swap the modules
        for m in (net.exclusive_net.net1, net.exclusive_net.net2):
            m.activation = act
            for i in range(1, len(m.net), 2):
                m.net[i] = getattr(torch.nn, act)()
        mlp = net.dimwise_net.net
        mlp.activation_name = act
        for i in range(1, len(mlp.net), 2):
            mlp.net[i] = getattr(torch.nn, act)()
    net = net.double()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(4, D, dtype=torch.float64)
    lat = torch.randn(4, L, dtype=torch.float64)
    f, jac = xt.closed_form(net, 0.3, x, lat)
    f64 = eh.net64(net, lat)
    J = torch.autograd.functional.jacobian(lambda v: f64(0.3, v).sum(0), x)             # [D, 4, D]: rows are independent
    want = torch.stack([J[i, :, i] for i in range(D)], -1)
    torch.testing.assert_close(f, f64(0.3, x), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(jac, want, rtol=1e-12, atol=1e-14)
    assert xt.closed_form(net, 0.3, x, lat, want_jac=False)[1] is None


def test_kernel_image_layout():
    """The LDS image read back position by position: mask * weight lands where include/stribor_hip.h says, huge entries under a zero
    mask do not arrive, and the size is the plan's."""
    torch.manual_seed(5)
    D, d_h, L, hidden = 7, 3, 5, [40, 24]
    net = st.net.DiffeqExactTraceMLP(D, hidden, D, d_h, latent_dim=L)
    l0 = net.exclusive_net.net1.net[0]
    with torch.no_grad():
        l0.weight[l0.mask == 0] = 1e30
    s = xt.kernel_coverage(net, D, L)
    assert s is not None and s['d_h'] == d_h and s['hidden'] == hidden
    image, w_latent = xt.kernel_image(s)
    HT, OT = 2, 2
    made = HT * 1024 + HT * 32 + HT * HT * 1024 + HT * 32 + OT * HT * 1024 + OT * 32
    assert image.size == 2 * made + HT * 1024 + 3 * HT * 32 + HT * HT * 1024 + HT * 32 + HT * 32 + 32
    assert np.isfinite(image).all() and np.abs(image).max() < 1e3
    kmap = lambda r, h: (r & 3) + 8 * (r >> 2) + 4 * h

    def read(base, kt, row, col):                              # Wp[row][col] of an image of kt column tiles
        m, c, lr, lc = row // 32, col // 32, row % 32, col % 32
        r, h = next((r, h) for r in range(16) for h in (0, 1) if kmap(r, h) == lc)
        return image[base + (m * kt + c) * 1024 + (r >> 2) * 256 + (lr + 32 * h) * 4 + (r & 3)]
    W = (l0.mask * l0.weight.detach()).numpy()
    W[l0.mask.numpy() == 0] = 0
    for j in (0, 17, 39):
        for i in range(D):
            assert read(0, 1, j, kmap(i, 0)) == W[j, i]
    last = net.exclusive_net.net2.net[4]
    Wl = (last.mask * last.weight.detach()).numpy()
    base = made + HT * 1024 + HT * 32 + HT * HT * 1024 + HT * 32
    for kk in range(d_h):
        for i in range(D):
            pos = 32 * (kk >> 1) + kmap(i, kk & 1)
            assert read(base, HT, pos, 11) == Wl[kk * D + i, 11]
            assert image[base + OT * HT * 1024 + pos] == last.bias[kk * D + i].item()
    W1 = net.dimwise_net.net.net[0].weight.detach().numpy()
    base = 2 * made
    assert read(base, 1, 33, 0) == W1[33, 1]
    for kk in range(d_h):
        assert read(base, 1, 33, kmap(1 + (kk >> 1), kk & 1)) == W1[33, 2 + kk]
    assert w_latent.shape == (64, 32) and np.array_equal(w_latent[:40, :L], W1[:, 2 + d_h:]) and not w_latent[40:].any()
    for bad in (st.net.DiffeqExactTraceMLP(17, [8], 17, 2), st.net.DiffeqExactTraceMLP(3, [65], 3, 2), st.net.DiffeqExactTraceMLP(3, [], 3, 2),
                st.net.DiffeqExactTraceMLP(3, [8, 8, 8], 3, 2), st.net.DiffeqExactTraceMLP(3, [8], 3, 9)):
        assert xt.kernel_coverage(bad, bad.exclusive_net.net1.in_dim, 0) is None
    assert xt.kernel_coverage(st.net.DiffeqExactTrace(net.exclusive_net, net.dimwise_net), D, L) is None
