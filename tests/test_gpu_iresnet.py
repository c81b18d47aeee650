"""GPU: IResNet / ContinuousIResNet (stribor/flows/iresnet.py) on sx_resnet_flow + sx_spectral_sigma.

Values against fixture F14 (tests/golden/make_golden_iresnet.py, captured from the reference): forward, the 100-step inverse,
the unconverged 7-step inverse, eval mode, and the spectral-norm state (u, v, weight) after every call; test_neural_flow.py
restated on the product; the one-launch contract; kernel vs composition fallback; gradients against fp64 autograd.
"""
import copy

import pytest
import torch
import torch.nn as nn

import flowdesc as fd
from goldens import Golden
from producthelp import close

import stribor_amd as st
from stribor_amd import _hip

pytestmark = pytest.mark.gpu
DEV = 'cuda'

F14 = None


def f14():
    global F14
    if F14 is None:
        F14 = Golden('f14_iresnet')
    return F14


def grid_cases():
    return sorted(c for c in Golden('f14_iresnet').meta if c.startswith('grid/'))


def _product(desc, state):
    f = fd.build_transform(st, desc)
    f.load_state_dict(state)
    return f.to(DEV)


def _check_sn(f, g, prefix, atol=1e-5):
    """u, v (unit vectors: absolute 1e-5) and the plain weight attribute after a call."""
    keys = [k for k in g.arrays if k.startswith(prefix + '/')]
    assert keys or not any(hasattr(m, 'weight_orig') for m in f.modules()), prefix
    mods = dict(f.named_modules())
    for k in keys:
        name, attr = k[len(prefix) + 1:].rsplit('.', 1)
        got = getattr(mods[name], attr)
        want = g.t(k)
        if attr == 'weight':
            close(got, want)
        else:
            close(got, want, rtol=0, atol=atol)


def _warm(f, t=False, n=5):
    """A few training-mode calls, as the reference's tests make: the power iteration settles and sigma bounds the Lipschitz
    constant (a freshly initialised u, v under-estimate it, and the fixed-point map need not contract)."""
    mode = f.training
    f.train(True)
    dim = f.dim
    with torch.no_grad():
        for _ in range(n):
            x = torch.randn(16, dim, device=DEV)
            f(x, t=torch.rand(16, 1, device=DEV)) if t else f(x)
    f.train(mode)
    return f


@pytest.mark.parametrize('case', grid_cases())
def test_grid_against_reference(case):
    g = f14()
    m = g.meta[case]
    f = _product(m['desc'], g.state(case))
    x = g.t(f'{case}/x').to(DEV)
    cont = g.has(f'{case}/t')
    kw = {'t': g.t(f'{case}/t').to(DEV)} if cont else {}
    with torch.no_grad():
        close(f(x, **kw), g.t(f'{case}/y'))
        _check_sn(f, g, f'{case}/after_y')
        y = g.t(f'{case}/y').to(DEV)
        close(f.inverse(y, **kw), g.t(f'{case}/x_back'))
        _check_sn(f, g, f'{case}/after_x_back')
        close(f.inverse(y, iterations=7, **kw), g.t(f'{case}/x_7'))
        _check_sn(f, g, f'{case}/after_x_7')
        f.eval()
        close(f(x, **kw), g.t(f'{case}/y_eval'))
        close(f.inverse(g.t(f'{case}/y_eval').to(DEV), **kw), g.t(f'{case}/x_back_eval'))
        _check_sn(f, g, f'{case}/after_x_7')                  # eval mode: no update
        if cont:
            y0 = f(x, t=torch.zeros_like(kw['t']))
            assert torch.equal(y0, x)
            assert torch.equal(y0.cpu(), g.t(f'{case}/y_zero'))


def test_time_zero_is_bitwise_identity_in_training_mode():
    torch.manual_seed(5)
    for tn in (st.net.TimeTanh(64), st.net.TimeFourierBounded(64, 8), st.net.TimeLinear(64)):
        f = st.ContinuousIResNet(64, [64, 64], time_net=tn).to(DEV)
        x = torch.randn(1000, 64, device=DEV)
        with torch.no_grad():
            assert torch.equal(f(x, t=torch.zeros(1000, 1, device=DEV)), x)


@pytest.mark.parametrize('case', ['kernel/64/ReLU', 'kernel/64/Tanh', 'kernel/128/ReLU', 'kernel/128/Tanh'])
def test_kernel_sized_cases(case):
    g = Golden('f14_iresnet_wide')
    m = g.meta[case]
    torch.manual_seed(m['seed'])
    f = fd.build_transform(st, m['desc'])
    f = f.to(DEV)
    torch.manual_seed(m['seed'] + 1)
    x = torch.randn(256, m['desc']['dim'])
    t = torch.rand(256, 1)
    kw = {'t': t.to(DEV)} if m['desc']['kind'] == 'continuous_iresnet' else {}
    with torch.no_grad():
        close(f(x.to(DEV), **kw), g.t(f'{case}/y'))
        _check_sn(f, g, f'{case}/after_y')
        close(f.inverse(g.t(f'{case}/y').to(DEV), **kw), g.t(f'{case}/x_back'))
        _check_sn(f, g, f'{case}/after_x_back')


def _neural_flow(g):
    m = g.meta['neural_flow']
    nf = st.NeuralFlow([fd.build_transform(st, d) for d in m['desc']])
    nf.load_state_dict(g.state('neural_flow'))
    return nf.to(DEV)


def test_neural_flow_restated():
    """test_neural_flow.py:4-30 on product modules from F14's state."""
    g = f14()
    nf = _neural_flow(g)
    x = g.t('neural_flow/x').to(DEV)
    with torch.no_grad():
        y = nf(x, t=torch.zeros_like(x[..., :1]))
        assert (x == y).all()
        assert torch.equal(y.cpu(), g.t('neural_flow/y_zero'))
        _check_sn(nf, g, 'neural_flow/after_y_zero')
        t0 = g.t('neural_flow/t0').to(DEV)
        y = nf(x, t=t0, t0=t0)
        assert torch.allclose(x, y)
        close(y, g.t('neural_flow/y_round_trip'))
        _check_sn(nf, g, 'neural_flow/after_y_round_trip')
        y = nf(x, t=g.t('neural_flow/t1').to(DEV), t0=t0)
        close(y, g.t('neural_flow/y_t1_t0'))
        _check_sn(nf, g, 'neural_flow/after_y_t1_t0')


def test_neural_flow_with_grad_enabled_round_trips():
    """The reference's own test runs in grad mode: the forward composes torch ops, the inverse is the implicit-gradient op."""
    g = f14()
    nf = _neural_flow(g)
    x = g.t('neural_flow/x').to(DEV)
    assert (nf(x, t=torch.zeros_like(x[..., :1])) == x).all()
    t0 = g.t('neural_flow/t0').to(DEV)
    y = nf(x, t=t0, t0=t0)
    assert y.requires_grad and torch.allclose(x, y)


@pytest.mark.parametrize('training', [True, False])
def test_one_launch(monkeypatch, training):
    torch.manual_seed(0)
    f = st.ContinuousIResNet(64, [64, 64], time_net=st.net.TimeTanh(64)).to(DEV)
    f.train(training)
    y = torch.randn(4096, 64, device=DEV)
    t = torch.rand(4096, 1, device=DEV)
    calls = []
    real = _hip.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(_hip, 'call', spy)
    with torch.no_grad():
        f.inverse(y, t=t)
    assert calls.count('sx_resnet_flow') == 1
    assert calls.count('sx_spectral_sigma') <= 1
    assert set(calls) <= {'sx_resnet_flow', 'sx_spectral_sigma'}, calls


class _SinTime(nn.Module):
    """A time net the kernel does not know: evaluated by torch, passed to the kernel as rows."""

    def __init__(self, dim):
        super().__init__()
        self.w = nn.Parameter(torch.randn(1, dim))

    def forward(self, t):
        return torch.sin(self.w * t) * t


@pytest.mark.parametrize('variant', ['relu', 'tanh_sigmoid', 'fourier', 'rows_time', 'three_hidden', 'empty', 'dim100'])
@pytest.mark.parametrize('training', [True, False])
def test_kernel_matches_composition(variant, training):
    torch.manual_seed(11)
    dim, hidden, kw = 64, [64, 64], {}
    if variant == 'tanh_sigmoid':
        kw = dict(activation='Tanh', final_activation='Sigmoid')
    tn = st.net.TimeTanh(dim)
    if variant == 'fourier':
        tn = st.net.TimeFourier(dim, 6)
    if variant == 'rows_time':
        tn = _SinTime(dim)
    if variant == 'three_hidden':
        hidden = [48, 64, 32]
        kw = dict(activation='SiLU')
    if variant == 'empty':
        hidden = []
    if variant == 'dim100':
        dim, hidden, tn = 100, [128], st.net.TimeLog(100)
    f = _warm(st.ContinuousIResNet(dim, hidden, time_net=tn, **kw).to(DEV), t=True).train(training)
    assert f._kernel_net() is not None
    h = copy.deepcopy(f)
    y = torch.randn(777, dim, device=DEV) * 2
    t = torch.rand(777, 1, device=DEV)
    with torch.no_grad():
        got = f.inverse(y, t=t)
        want = h._composed_reference(y, t)
        close(got, want)
        for (na, a), (nb, b) in zip(f.named_buffers(), h.named_buffers()):
            close(a, b, rtol=0, atol=1e-5)
        close(f(y, t=t), h._composed_reference(y, t, inverse=False))


def test_fallback_outside_kernel_coverage():
    """A custom activation and a wider net run the composition fallback with the same schedule."""
    torch.manual_seed(3)
    for f in (st.IResNet(16, [32], activation='Hardtanh'), st.IResNet(16, [256])):
        f = f.to(DEV)
        assert f._kernel_net() is None
        y = torch.randn(100, 16, device=DEV)
        with torch.no_grad():
            x = f.inverse(y)
            assert torch.allclose(f(x), y, atol=1e-4)


def test_other_dtypes_raise():
    f = st.IResNet(4, [8]).to(DEV)
    with pytest.raises(TypeError):
        f(torch.randn(3, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(TypeError):
        f.inverse(torch.randn(3, 4, device=DEV, dtype=torch.bfloat16))


@pytest.mark.parametrize('n', [1, 33, 4097, 1 << 20])
def test_sizes(n):
    torch.manual_seed(n % 1000)
    f = _warm(st.IResNet(64, [64, 64]).to(DEV)).eval()
    y = torch.randn(n, 64, device=DEV)
    with torch.no_grad():
        got = f.inverse(y)
        want = f._composed_reference(y)
    close(got, want)


# ---- gradients ----------------------------------------------------------------------------------------------------------
def _params64(f):
    """fp64 copies of the network's tensors: [(W_orig or W, b, u, v, n_power or None)], time-net scale."""
    out = []
    for m in f.net.net:
        if isinstance(m, nn.Linear):
            if hasattr(m, 'weight_orig'):
                out.append([m.weight_orig.detach().double().requires_grad_(), m.bias.detach().double().requires_grad_(),
                            m.weight_u.detach().double().clone(), m.weight_v.detach().double().clone()])
            else:
                out.append([m.weight.detach().double().requires_grad_(), m.bias.detach().double().requires_grad_(), None, None])
    return out


def _g64(layers, x, n_power, act=torch.relu):
    """The reference's MLP with spectral_norm restated in fp64; `n_power` rounds advance the u / v held in `layers`."""
    h = x
    for i, L in enumerate(layers):
        W, b, u, v = L
        if u is not None:
            with torch.no_grad():
                for _ in range(n_power):
                    v = nn.functional.normalize(W.t().mv(u), dim=0, eps=1e-12)
                    u = nn.functional.normalize(W.mv(v), dim=0, eps=1e-12)
            L[2], L[3] = u, v
            W = W / torch.dot(u, W.mv(v))
        h = nn.functional.linear(h, W, b)
        if i + 1 < len(layers):
            h = act(h)
    return h


@pytest.mark.parametrize('training', [False, True])
def test_forward_gradients_vs_fp64(training):
    torch.manual_seed(21)
    f = _warm(st.ContinuousIResNet(8, [32, 32], time_net=st.net.TimeTanh(8)).to(DEV), t=True).train(training)
    x = torch.randn(50, 8, device=DEV, requires_grad=True)
    t = torch.rand(50, 1, device=DEV, requires_grad=True)
    cot = torch.randn(50, 8, device=DEV)
    layers = _params64(f)
    scale = f.time_net.scale.detach().double().requires_grad_()
    x64, t64 = x.detach().double().requires_grad_(), t.detach().double().requires_grad_()
    y = f(x, t=t)
    (y * cot).sum().backward()
    y64 = x64 + torch.tanh(scale * t64) * _g64(layers, x64, 5 if training else 0)
    (y64 * cot.double()).sum().backward()
    close(y, y64)
    close(x.grad, x64.grad)
    close(t.grad, t64.grad)
    close(f.time_net.scale.grad, scale.grad)
    lins = [m for m in f.net.net if isinstance(m, nn.Linear)]
    for m, L in zip(lins, layers):
        close(getattr(m, 'weight_orig', None).grad if hasattr(m, 'weight_orig') else m.weight.grad, L[0].grad)
        close(m.bias.grad, L[1].grad)


@pytest.mark.parametrize('training', [False, True])
def test_inverse_gradients_vs_unrolled_fp64(training):
    torch.manual_seed(22)
    f = _warm(st.ContinuousIResNet(8, [32, 32], time_net=st.net.TimeTanh(8)).to(DEV), t=True).train(training)
    y = torch.randn(50, 8, device=DEV, requires_grad=True)
    t = torch.rand(50, 1, device=DEV, requires_grad=True)
    cot = torch.randn(50, 8, device=DEV)
    layers = _params64(f)
    scale = f.time_net.scale.detach().double().requires_grad_()
    y64, t64 = y.detach().double().requires_grad_(), t.detach().double().requires_grad_()
    x = f.inverse(y, t=t)
    (x * cot).sum().backward()
    s64 = torch.tanh(scale * t64)
    x64 = y64
    for _ in range(100):                                        # iresnet.py:86-89, unrolled
        x64 = y64 - s64 * _g64(layers, x64, 5 if training else 0)
    (x64 * cot.double()).sum().backward()
    close(x, x64)
    close(y.grad, y64.grad, rtol=1e-4, atol=1e-4)
    close(t.grad, t64.grad, rtol=1e-4, atol=1e-4)
    close(f.time_net.scale.grad, scale.grad, rtol=1e-4, atol=1e-4)
    lins = [m for m in f.net.net if isinstance(m, nn.Linear)]
    for m, L in zip(lins, layers):
        close(m.weight_orig.grad if hasattr(m, 'weight_orig') else m.weight.grad, L[0].grad, rtol=1e-4, atol=1e-4)
        close(m.bias.grad, L[1].grad, rtol=1e-4, atol=1e-4)


def test_iresnet_inverse_gradient_without_time():
    torch.manual_seed(23)
    f = _warm(st.IResNet(4, [16]).to(DEV)).eval()
    y = torch.randn(20, 4, device=DEV, requires_grad=True)
    x = f.inverse(y)
    x.sum().backward()
    layers = _params64(f)
    y64 = y.detach().double().requires_grad_()
    x64 = y64
    for _ in range(100):
        x64 = y64 - _g64(layers, x64, 0)
    x64.sum().backward()
    close(y.grad, y64.grad, rtol=1e-4, atol=1e-4)
