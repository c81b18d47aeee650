"""Host (no GPU): the attention nets' surface (stribor/net/attention.py:8-147, util/safe_softmax.py) -- constructor signatures,
state_dict keys, the default init under every F15 seed against the reference's sha256 (tests/golden/make_golden_attention.py),
the flow-description conditioner kinds, safe_softmax, and that CPU tensors raise (there is no CPU fallback); the fp64 oracle of
test_gpu_attention_core.py (attncorehelp.oracle) against the fp64 composition on every case of that module, and the conditions on
those cases."""
import hashlib
import inspect

import numpy as np
import pytest
import torch

import attncorehelp as ach
import flowdesc as fd
from goldens import Golden

import stribor_amd as st
from stribor_amd import _hip

F15 = Golden('f15_attention')


def _sha(t):
    a = np.ascontiguousarray(t.detach().numpy())
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def _params(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


def test_exports():
    for name in ('attention', 'Attention', 'SelfAttention', 'InducedSelfAttention'):
        assert hasattr(st.net, name), name
    assert callable(st.util.safe_softmax)
    assert 'SelfAttention' in st.__doc__ and 'safe_softmax' in st.__doc__
    assert {'sx_attention_fwd', 'sx_attention_bwd'} <= set(_hip.EXPORTS)


def test_constructor_and_forward_signatures_match_the_reference():
    E = inspect.Parameter.empty
    assert _params(st.net.attention) == [('query', E), ('key', E), ('value', E), ('n_heads', 1), ('mask_diagonal', False),
                                         ('mask', None)]
    assert _params(st.net.Attention.__init__) == [('self', E), ('in_dim', E), ('hidden_dims', E), ('out_dim', E), ('n_heads', 1),
                                                  ('mask_diagonal', False), ('kwargs', E)]
    assert _params(st.net.SelfAttention.__init__) == [('self', E), ('in_dim', E), ('hidden_dim', E), ('out_dim', E),
                                                      ('n_heads', 1), ('mask_diagonal', False), ('kwargs', E)]
    assert _params(st.net.InducedSelfAttention.__init__) == [('self', E), ('in_dim', E), ('hidden_dim', E), ('out_dim', E),
                                                             ('n_heads', 1), ('n_points', 32), ('kwargs', E)]
    assert _params(st.net.Attention.forward)[:5] == [('self', E), ('query', E), ('key', E), ('value', E), ('mask', None)]
    assert _params(st.net.SelfAttention.forward)[:3] == [('self', E), ('x', E), ('mask', None)]
    assert _params(st.net.InducedSelfAttention.forward)[:3] == [('self', E), ('x', E), ('mask', None)]
    assert _params(st.util.safe_softmax) == [('x', E), ('dim', -1)]


def test_state_dict_keys():
    a = st.net.SelfAttention(3, [64, 32], 5, n_heads=4)
    assert list(a.state_dict()) == ['key.net.0.weight', 'key.net.0.bias', 'key.net.2.weight', 'key.net.2.bias',
                                    'query.net.0.weight', 'query.net.0.bias', 'query.net.2.weight', 'query.net.2.bias',
                                    'value.net.0.weight', 'value.net.0.bias', 'value.net.2.weight', 'value.net.2.bias',
                                    'proj.weight', 'proj.bias']
    i = st.net.InducedSelfAttention(3, [32], 5, n_points=7)
    keys = list(i.state_dict())
    assert keys[0] == 'points' or keys[-1] == 'points'
    assert [k for k in keys if k != 'points'] == ['att1.' + k for k in st.net.Attention(3, [32], 3).state_dict()] + \
        ['att2.' + k for k in st.net.Attention(3, [32], 5).state_dict()]
    assert i.points.shape == (7, 3) and i.att1.proj.weight.shape == (3, 32) and i.att2.proj.weight.shape == (5, 32)


def kernel_model(model, N, heads):
    """The F15 kernel-sized models (make_golden_attention.py: kernel_model)."""
    if model == 'SelfAttention':
        return st.net.SelfAttention(4, [64], 3, n_heads=heads, mask_diagonal=heads == 4)
    return st.net.InducedSelfAttention(4, [64], 3, n_heads=heads, n_points=N if N == 33 else 16)


def _check_hashes(m, want, case):
    state = m.state_dict()
    assert set(state) == set(want), (case, sorted(set(state) ^ set(want)))
    for k, v in state.items():
        assert _sha(v) == want[k], f'{case}: {k} differs from the reference\'s default init'


def test_grid_default_init_matches_the_reference():
    """Every init configuration of test_attention.py's grid under torch.manual_seed(123): same draws, same order."""
    cases = F15.cases('init/')
    assert len(cases) == 3 * 4 * 2 * 3
    for case in cases:
        _, model, in_dim, h, out = case.split('/')
        hidden = [32] if h == 'h1' else [64, 32]
        torch.manual_seed(123)
        m = getattr(st.net, model)(int(in_dim), hidden, int(out[1:]), n_heads=4, mask_diagonal=True, n_points=11)
        _check_hashes(m, F15.meta[case]['state_sha256'], case)


def test_kernel_and_flow_default_init_matches_the_reference():
    for case in F15.cases('kernel/'):
        _, model, n, h = case.split('/')
        torch.manual_seed(F15.meta[case]['seed'])
        m = kernel_model(model, int(n[1:]), int(h[1:]))
        _check_hashes(m, F15.meta[case]['state_sha256'], case)
    for case in F15.cases('flow/'):
        meta = F15.meta[case]
        torch.manual_seed(meta['seed'])
        flow = fd.build_flow(st, meta['desc'], meta['dim'])
        _check_hashes(flow, meta['state_sha256'], case)
        net = flow.transforms[0].transform.latent_net
        assert isinstance(net, (st.net.SelfAttention, st.net.InducedSelfAttention))


def test_safe_softmax():
    x = torch.tensor([[0., 1., -float('inf')], [-float('inf')] * 3])
    y = st.util.safe_softmax(x, -1)
    assert torch.equal(y[1], torch.zeros(3))
    assert torch.allclose(y[0], torch.softmax(x[0], -1))


def _heads_scores(q, k, H):
    """[..., H, Nq, Nk] fp64 logits, written apart from attncorehelp.oracle's per-head loop."""
    dh = q.shape[-1] // H
    qh = q.double().reshape(*q.shape[:-1], H, dh).transpose(-2, -3)
    kh = k.double().reshape(*k.shape[:-1], H, dh).transpose(-2, -3)
    return qh @ kh.transpose(-1, -2) / dh ** 0.5


def _oracle_against_composition(c, t, masked, diag, tag):
    """y, dq, dk, dv of attncorehelp's oracle against fp64 _attention_composed to 1e-12, its lse against fp64 logsumexp over the
    live keys; the fp32 composition (the GPU tests' error yardstick) is finite."""
    from stribor_amd.net.attention import _attention_composed
    mask = c['mask'] if masked else None
    q, k, v = (c[n].double().requires_grad_() for n in 'qkv')
    y = _attention_composed(q, k, v, c['n_heads'], diag, None if mask is None else mask.double())
    grads = torch.autograd.grad(y, (q, k, v), c['gy'].double())
    for n, want in zip(('y', 'dq', 'dk', 'dv'), (y.detach(),) + grads):
        assert t[n].dtype == torch.float64 and t[n].shape == want.shape
        err = (t[n] - want).abs().max().item()
        assert err <= 1e-12, (tag, n, err)
    s = _heads_scores(c['q'], c['k'], c['n_heads'])
    if mask is not None:
        s = s.masked_fill((mask[..., 0] != 1)[:, None, None, :], -float('inf'))
    if diag:
        s = s.masked_fill(torch.eye(s.shape[-1], dtype=torch.bool), -float('inf'))
    want = torch.logsumexp(s, -1)
    dead = torch.isinf(want)                                   # (-inf: no live key)
    assert torch.equal(torch.isinf(t['lse']) & (t['lse'] > 0), dead), tag
    assert (t['lse'][~dead] - want[~dead]).abs().max().item() <= 1e-12, tag
    y32 = _attention_composed(c['q'], c['k'], c['v'], c['n_heads'], diag, mask)
    assert y32.dtype == torch.float32 and torch.isfinite(y32).all(), tag


@pytest.mark.parametrize('name', sorted(ach.CASES))
def test_core_oracle_matches_the_fp64_composition(name):
    """Every case of test_gpu_attention_core.py's sweep: the independent oracle against the composition, and the conditions that
    keep the sweep from being trivial (attncorehelp.check_conditions)."""
    ach.check_conditions(name)
    for masked, diag in ach.runs(name):
        _oracle_against_composition(ach.case(name), ach.truth(name, masked, diag), masked, diag, (name, masked, diag))


@pytest.mark.parametrize('shape', sorted(ach.LOGIT_SHAPES))
@pytest.mark.parametrize('variant', ach.LOGIT_VARIANTS)
def test_core_oracle_on_large_and_shifted_logits(shape, variant):
    """The large-logit cases: their construction holds (tile maxima monotone, shift of order 300), the oracle still agrees with the
    fp64 composition, the fp32 composition stays finite, and the shift leaves the fp64 result where it was."""
    ach.check_logit_conditions(shape, variant)
    c = ach.logit_case(shape, variant)
    for masked in (False, True):
        _oracle_against_composition(c, ach.logit_truth(shape, variant, masked), masked, False, (shape, variant, masked))
    if variant == 'shift300':
        y0, _ = ach.oracle(c['q'], c['k'].double() - c['shift'].double(), c['v'], c['n_heads'], False, None)
        assert (ach.logit_truth(shape, variant, False)['y'] - y0).abs().max().item() <= 1e-9


def test_core_oracle_edges():
    """The oracle's own edges: a query without a live key gives y = 0 and lse = +inf, 0.5 is dead, the output mask is the raw value,
    no key at all."""
    q, k, v = torch.randn(2, 3, 4), torch.randn(2, 3, 4), torch.randn(2, 3, 4)
    mask = torch.tensor([[1., 0.5, 0.], [0., 0., 0.5]]).unsqueeze(-1)
    y, lse = ach.oracle(q, k, v, 2, False, mask)
    assert torch.equal(y[1], torch.zeros(3, 4, dtype=torch.float64)) and torch.equal(lse[1], torch.full((2, 3), float('inf')).double())
    assert torch.allclose(y[0, 0], v[0, 0].double()) and torch.allclose(y[0, 1], 0.5 * v[0, 0].double())
    assert torch.equal(y[0, 2], torch.zeros(4, dtype=torch.float64))
    s = _heads_scores(q, k, 2)
    assert torch.allclose(lse[0], s[0, :, :, 0])
    y, lse = ach.oracle(q, k, v, 1, True, mask)
    assert torch.equal(y[0, 0], torch.zeros(4, dtype=torch.float64)) and torch.isinf(lse[0, 0, 0]) and torch.isfinite(lse[0, 0, 1:]).all()
    y, lse = ach.oracle(q, k[:, :0], v[:, :0], 2, False, None)
    assert torch.equal(y, torch.zeros(2, 3, 4, dtype=torch.float64)) and torch.isinf(lse).all() and (lse > 0).all()


def test_cpu_tensors_raise():
    x = torch.randn(2, 5, 8)
    with pytest.raises(RuntimeError, match='ROCm device'):
        st.net.attention(x, x, x, n_heads=2)
    for m in (st.net.SelfAttention(8, [16], 3, n_heads=2), st.net.InducedSelfAttention(8, [16], 3, n_heads=2, n_points=4)):
        with pytest.raises(RuntimeError, match='ROCm device'):
            m(x)
    with pytest.raises(RuntimeError, match='ROCm device'):
        st.net.Attention(8, [16, 16], 3)(x, x, x)
