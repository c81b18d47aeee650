"""GPU: the attention nets (stribor/net/attention.py:8-147) on the HIP attention core (sx_attention_fwd / sx_attention_bwd).

Values against fixture F15 (tests/golden/make_golden_attention.py, captured from the reference): test_attention.py's grid for all
three models and kernel-sized sets (masked, non-binary and fully masked sets, mask_diagonal, the n_points == N quirk), with
test_attention.py's equivariance and masking assertions restated on the product; the one-launch contract and the no-N x N memory
bound; gradients against fp64 autograd of the torch composition, bit-reproducible; the dh > 128 composition; a 3-layer set flow
(values and fp64 parameter gradients from the reference); HIP graph replay.
"""
import warnings

import pytest
import torch

import flowdesc as fd
from goldens import Golden
from producthelp import close

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.net.attention import _attention_composed

pytestmark = pytest.mark.gpu
DEV = 'cuda'

F15 = Golden('f15_attention')


def _grid_cases():
    return F15.cases('grid/')


def _call(model, name, x, mask=None):
    if name == 'Attention':
        return model(x, x, x, mask) if mask is not None else model(x, x, x)
    return model(x, mask) if mask is not None else model(x)


@pytest.mark.parametrize('model_name', ['Attention', 'SelfAttention', 'InducedSelfAttention'])
def test_f15_grid_values_equivariance_and_masking(model_name):
    """test_attention.py:5-49 on the device: the reference's outputs (unmasked and masked), permutation equivariance, and that
    masked elements' values do not change the output."""
    cases = [c for c in _grid_cases() if c.split('/')[1] == model_name]
    assert len(cases) == 4 * 2 * 3 * 3 * 2
    for case in cases:
        _, _, shp, h, o, H, d = case.split('/')
        shp = tuple(int(s) for s in shp.split('x'))
        hidden = [32] if h == 'h1' else [64, 32]
        torch.manual_seed(123)                                   # the reference test's stream, drawn on the host
        m = getattr(st.net, model_name)(shp[-1], hidden, int(o[1:]), n_heads=int(H[1:]), mask_diagonal=d == 'd1', n_points=11)
        x = torch.randn(*shp)
        mask = torch.rand(*shp[:-1], 1).round()
        mask[..., 0, 0] = 1
        x_perm = x + x * (1 - mask) * torch.rand(*shp)
        m = m.to(DEV)
        x, mask, x_perm = x.to(DEV), mask.to(DEV), x_perm.to(DEV)
        with torch.no_grad():
            y = _call(m, model_name, x)
            y_mask = _call(m, model_name, x, mask)
            close(y, F15.t(f'{case}/y'))
            close(y_mask, F15.t(f'{case}/y_mask'))
            y_flip = torch.flip(_call(m, model_name, torch.flip(x, [-2])), [-2])
            assert torch.isclose(y, y_flip, atol=1e-5).all(), case
            assert torch.isclose(y_mask, _call(m, model_name, x_perm, mask), atol=1e-5).all(), case
            assert not torch.isnan(y).any() and not torch.isnan(y_mask).any()


def _kernel_model(model, N, heads):
    if model == 'SelfAttention':
        return st.net.SelfAttention(4, [64], 3, n_heads=heads, mask_diagonal=heads == 4)
    return st.net.InducedSelfAttention(4, [64], 3, n_heads=heads, n_points=N if N == 33 else 16)


def _kernel_mask(N):
    m = torch.ones(3, N, 1)
    m[1, :, 0] = torch.floor(torch.rand(N) * 3) / 2
    m[1, 0, 0] = 1
    m[2] = 0
    return m


def test_f15_kernel_sized_sets():
    """N in {1, 31, 33, 64, 257}, E = 64, 1 / 4 heads: masked, non-binary (0.5) and fully masked sets, mask_diagonal, and
    InducedSelfAttention with n_points == N (the output mask of attention.py:47-48 then applies to att1)."""
    cases = F15.cases('kernel/')
    assert len(cases) == 2 * 5 * 2
    for case in cases:
        _, model, n, h = case.split('/')
        N = int(n[1:])
        torch.manual_seed(F15.meta[case]['seed'])
        m = _kernel_model(model, N, int(h[1:]))
        x = torch.randn(3, N, 4)
        mask = _kernel_mask(N)
        m = m.to(DEV)
        with torch.no_grad():
            close(m(x.to(DEV)), F15.t(f'{case}/y'))
            close(m(x.to(DEV), mask.to(DEV)), F15.t(f'{case}/y_mask'))


@pytest.mark.parametrize('N,E,H', [(1, 64, 1), (33, 64, 4), (257, 64, 4), (40, 96, 1), (20, 8, 8), (17, 6, 2)])
def test_core_masking_rules(N, E, H):
    """The core against the torch composition: masked keys (mask != 1, 0.5 included), the output mask when Nq == Nk, fully masked
    sets give exactly 0 and no NaN, mask_diagonal (with N = 1 every query is masked)."""
    g = torch.Generator().manual_seed(N + E + H)
    q, k, v = (torch.randn(4, N, E, generator=g).to(DEV) for _ in range(3))
    mask = (torch.floor(torch.rand(4, N, 1, generator=g) * 3) / 2)
    mask[0] = 1
    mask[1, 0] = 1
    mask[3] = 0
    mask = mask.to(DEV)
    for diag in (False, True):
        for mk in (None, mask):
            with torch.no_grad():
                y = st.net.attention(q, k, v, n_heads=H, mask_diagonal=diag, mask=mk)
                want = _attention_composed(q.double(), k.double(), v.double(), H, diag, None if mk is None else mk.double())
            assert not torch.isnan(y).any()
            close(y, want, rtol=1e-5, atol=1e-5)
            if mk is not None:
                assert torch.equal(y[3], torch.zeros_like(y[3]))       # fully masked set: exactly 0
            if diag and N == 1:
                assert torch.equal(y, torch.zeros_like(y))


def test_core_queries_unlike_keys_and_errors():
    g = torch.Generator().manual_seed(5)
    q = torch.randn(2, 3, 11, 32, generator=g).to(DEV)
    k, v = (torch.randn(2, 3, 40, 32, generator=g).to(DEV) for _ in range(2))
    mask = torch.rand(2, 3, 40, 1, generator=g).round().to(DEV)
    with torch.no_grad():
        y = st.net.attention(q, k, v, n_heads=4, mask=mask)
    close(y, _attention_composed(q.double(), k.double(), v.double(), 4, False, mask.double()))
    with pytest.raises(RuntimeError):
        st.net.attention(q, k, v, n_heads=4, mask_diagonal=True)          # Nq != Nk
    with pytest.raises(RuntimeError):
        st.net.attention(k, k, v, n_heads=3)                              # 3 does not divide 32
    with pytest.raises(NotImplementedError):
        st.net.attention(k, k, v, n_heads=4, mask=torch.ones(2, 3, 40, 1, device=DEV, requires_grad=True))
    e = torch.zeros(0, 5, 32, device=DEV)
    assert st.net.attention(e, e, e, n_heads=4).shape == (0, 5, 32)
    z = torch.zeros(3, 0, 32, device=DEV)
    assert torch.equal(st.net.attention(q[0], z, z, n_heads=4), torch.zeros(3, 11, 32, device=DEV))


def test_one_launch(monkeypatch):
    x = torch.randn(64, 33, 64, device=DEV)
    calls = []
    real = _hip.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(_hip, 'call', spy)
    with torch.no_grad():
        st.net.attention(x, x, x, n_heads=4, mask=torch.ones(64, 33, 1, device=DEV))
    assert calls == ['sx_attention_fwd'], calls


def test_no_score_tensor_in_memory():
    """(16, 4096, 64, 4): the [16, 4, 4096, 4096] score tensor would be 4.3 GB; forward and forward + backward stay < 128 MB."""
    B, N, E, H = 16, 4096, 64, 4
    q, k, v = (torch.randn(B, N, E, device=DEV, requires_grad=True) for _ in range(3))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        y = st.net.attention(q, k, v, n_heads=H)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 128 << 20
    del y
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = st.net.attention(q, k, v, n_heads=H)
    y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 128 << 20
    assert q.grad is not None and not torch.isnan(q.grad).any()


@pytest.mark.parametrize('N,E,H,masked,diag', [(31, 64, 4, True, False), (64, 64, 4, True, True), (257, 64, 1, True, False),
                                               (33, 128, 1, False, True), (9, 12, 3, True, False), (70, 256, 1, True, False)])
def test_core_gradients_match_fp64(N, E, H, masked, diag):
    """dq, dk, dv of the core against fp64 autograd of the composition; E = 256 with one head (dh = 256) is the composition
    fallback.  Two backward runs are bit-identical."""
    g = torch.Generator().manual_seed(N * E + H)
    B = 3
    q0, k0, v0 = (torch.randn(B, N, E, generator=g) for _ in range(3))
    gy = torch.randn(B, N, E, generator=g)
    mask = None
    if masked:
        mask = torch.floor(torch.rand(B, N, 1, generator=g) * 3) / 2
        mask[0, 0] = 1
        mask[2] = 0
    grads = []
    for _ in range(2):
        q, k, v = (t.to(DEV).requires_grad_() for t in (q0, k0, v0))
        y = st.net.attention(q, k, v, n_heads=H, mask_diagonal=diag, mask=None if mask is None else mask.to(DEV))
        y.backward(gy.to(DEV))
        grads.append([q.grad, k.grad, v.grad])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    q, k, v = (t.double().requires_grad_() for t in (q0, k0, v0))
    y = _attention_composed(q, k, v, H, diag, None if mask is None else mask.double())
    y.backward(gy.double())
    for got, want in zip(grads[0], (q.grad, k.grad, v.grad)):
        close(got, want, rtol=1e-4, atol=1e-6 * max(1.0, want.abs().max().item()))


def _composed_model_forward(m, x, mask):
    """SelfAttention / InducedSelfAttention with the torch composition in place of the core (fp64 parameters)."""
    def att(a, query, key, value, mask=None):
        return a.proj(_attention_composed(a.query.net(query), a.key.net(key), a.value.net(value), a.n_heads, a.mask_diagonal,
                                          mask))
    if isinstance(m, st.net.InducedSelfAttention):
        h = m.points.expand(*x.shape[:-2], *m.points.shape)
        h = att(m.att1, h, x, x, mask)
        return att(m.att2, x * (1 if mask is None else mask), h, h)
    return att(m, x, x, x, mask)


@pytest.mark.parametrize('model', ['SelfAttention', 'InducedSelfAttention'])
@pytest.mark.parametrize('hidden', [[64], [32, 64]])
def test_parameter_gradients_match_fp64(model, hidden):
    torch.manual_seed(7)
    m = (st.net.SelfAttention(5, hidden, 3, n_heads=4) if model == 'SelfAttention'
         else st.net.InducedSelfAttention(5, hidden, 3, n_heads=4, n_points=9))
    x = torch.randn(6, 33, 5)
    mask = torch.rand(6, 33, 1).round()
    mask[:, 0] = 1
    gy = torch.randn(6, 33, 3)
    md = m.to(DEV)
    xd = x.to(DEV).requires_grad_()
    y = md(xd, mask.to(DEV))
    y.backward(gy.to(DEV))
    got = {k: p.grad.clone() for k, p in md.named_parameters()}
    got['x'] = xd.grad
    m64 = md.to('cpu').double()
    m64.zero_grad(set_to_none=True)
    x64 = x.double().requires_grad_()
    y64 = _composed_model_forward(m64, x64, mask.double())
    close(y.detach(), y64.detach(), rtol=1e-5, atol=1e-5)
    y64.backward(gy.double())
    want = {k: p.grad for k, p in m64.named_parameters()}
    want['x'] = x64.grad
    for k in want:
        close(got[k], want[k], rtol=1e-4, atol=1e-6 * max(1.0, want[k].abs().max().item()))


@pytest.mark.parametrize('cond', ['self_attention', 'induced_self_attention'])
def test_f15_set_flow(cond):
    """A 3-layer set flow of Coupling(Affine(latent_net=<attention net>), set_data=True): log_prob, forward and inverse against the
    reference, and -log_prob.mean() parameter gradients against the reference's fp64 gradients, with no detached-graph warning."""
    case = f'flow/{cond}'
    meta = F15.meta[case]
    torch.manual_seed(meta['seed'])
    flow = fd.build_flow(st, meta['desc'], meta['dim'])
    x, latent = torch.randn(8, 16, 4), torch.randn(8, 16, 3)
    flow = flow.to(DEV)
    x, latent = x.to(DEV), latent.to(DEV)
    with torch.no_grad():
        close(flow.log_prob(x, latent=latent), F15.t(f'{case}/log_prob'))
        close(flow.forward(x, latent=latent), F15.t(f'{case}/forward'))
        close(flow.inverse(x, latent=latent), F15.t(f'{case}/inverse'))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        loss = -flow.log_prob(x, latent=latent).mean()
        loss.backward()
    close(loss.detach(), F15.t(f'{case}/loss64'), rtol=1e-5, atol=1e-5)
    for k, p in flow.named_parameters():
        want = F15.t(f'{case}/grad/{k}')
        close(p.grad, want, rtol=1e-4, atol=1e-6 * max(1.0, want.abs().max().item()))


def test_graph_replay_is_bit_identical():
    torch.manual_seed(3)
    m = st.net.SelfAttention(8, [64], 8, n_heads=4).to(DEV)
    static_x = torch.randn(256, 40, 8, device=DEV)
    static_mask = torch.rand(256, 40, 1, device=DEV).round()

    def step():
        with torch.no_grad():
            return m(static_x, static_mask)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static_out = step()
    for seed in range(2):
        static_x.copy_(torch.randn(256, 40, 8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)))
        graph.replay()
        torch.cuda.synchronize()
        got = static_out.clone()
        assert torch.equal(got, step())
