"""GPU: the slab forward tier's WIDE form -- rational-quadratic couplings of 17 .. 32 bins behind conditioners of 129 .. 256 hidden
units (sx_rqs_slab_hidden + sx_rqs_slab_wide_fwd: one transformed column per slab, each element in a lane pair).

Tolerances are the tier's own (test_spline_couplings_with_hidden_layers_beyond_128_take_the_slab_forward): log_prob / log-det rtol 1e-5
and atol 2e-4 * max(1, dim // 32), y atol 2e-5, round trip 1e-4.  Each error is also printed over cnfhelp.bound(oracle fp32, oracle
fp64) for the record."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import flowdesc as fd
from cnfhelp import bound
from producthelp import close

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import stribor_oracle as orc

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.flows.coupling import Coupling

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HALVES = ('ordered_right_half', 'ordered_left_half')
PARITY = ('parity_even', 'parity_odd')
SLAB_ENTRIES = ('sx_rqs_slab_fwd', 'sx_rqs_slab_wide_fwd')


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


@pytest.fixture
def spy(monkeypatch):
    """Counts the calls of Coupling._run_spline_slab that RETURN (a refusal enters and raises) and records the library entries called."""
    seen = {'returns': 0, 'entries': []}
    orig_run, orig_call = Coupling._run_spline_slab, _hip.call

    def run(self, *a):
        out = orig_run(self, *a)
        seen['returns'] += 1
        return out

    def call(name, *a, **kw):
        seen['entries'].append(name)
        return orig_call(name, *a, **kw)
    monkeypatch.setattr(Coupling, '_run_spline_slab', run)
    monkeypatch.setattr(_hip, 'call', call)
    return seen


def _flow(dim, hidden, K, masks, latent, layers=3, spline_type='quadratic', seed=None):
    torch.manual_seed(dim * 13 + hidden + K if seed is None else seed)
    desc = [{'kind': 'coupling_rqs', 'dim': dim, 'hidden': [hidden], 'n_bins': K, 'lower': -2.5, 'upper': 2.5, 'mask': masks[i % 2],
             'latent_dim': latent, 'spline_type': spline_type} for i in range(layers)]
    flow = fd.build_flow(st, desc, dim)
    spec = fd.flow_spec(desc, {k: v.clone() for k, v in flow.state_dict().items()})
    return flow.to(DEV), spec


def _report(what, got, ref32, ref64):
    b, e_ref = bound(ref32, ref64)
    err = (got.detach().double().cpu() - ref64).abs().max().item() if ref64.numel() else 0.0
    print(f'{what}: max |got - fp64| {err:.3e} = {err / b:.3f} x bound(oracle fp32, oracle fp64) {b:.3e} (oracle fp32 error {e_ref:.3e})')


PARITY_CASES = [(64, 160, 24, HALVES, 0), (33, 129, 17, HALVES, 7), (2, 130, 32, HALVES, 0), (48, 200, 31, PARITY, 0),
                (64, 256, 32, HALVES, 0)]


@pytest.mark.parametrize('dim,hidden,K,masks,latent', PARITY_CASES)
def test_wide_spline_couplings_take_the_slab_forward(dim, hidden, K, masks, latent, spy, monkeypatch):
    """Three-layer flows against the oracle in every direction, inputs reaching into the linear tails, ragged batches; every layer is
    answered by the slab tier through sx_rqs_slab_wide_fwd; and against the tier it replaces (the parameter tensor through HBM)."""
    flow, spec = _flow(dim, hidden, K, masks, latent)
    spec64 = orc.spec_to(spec, torch.float64)
    atol_l = 2e-4 * max(1, dim // 32)
    for n in (1, 300, 2049):
        x = torch.randn(n, dim) * 1.5
        lat = torch.randn(n, latent) if latent else None
        latd = None if lat is None else lat.to(DEV)
        l64 = None if lat is None else lat.double()
        want_lp, want_lp64 = orc.flow_log_prob(spec, x, lat), orc.flow_log_prob(spec64, x.double(), l64)
        (wy, wl), (wy64, wl64) = orc.flow_forward_and_ldj(spec, x, lat), orc.flow_forward_and_ldj(spec64, x.double(), l64)
        n0, e0 = spy['returns'], len(spy['entries'])
        lp = flow.log_prob(x.to(DEV), latent=latd)
        assert spy['returns'] == n0 + 3                                   # every layer answered by the slab tier
        assert spy['entries'][e0:].count('sx_rqs_slab_wide_fwd') == 3 and 'sx_rqs_slab_fwd' not in spy['entries'][e0:]
        y, ldj = flow.forward_and_log_det_jacobian(x.to(DEV), latent=latd)
        xr = flow.inverse(y, latent=latd)
        assert spy['returns'] == n0 + 9 and spy['entries'][e0:].count('sx_rqs_slab_wide_fwd') == 9
        _report(f'log_prob n={n}', lp, want_lp, want_lp64)
        _report(f'y n={n}', y, wy, wy64)
        _report(f'ldj n={n}', ldj, wl, wl64)
        close(lp, want_lp, rtol=1e-5, atol=atol_l)
        close(y, wy, rtol=1e-5, atol=2e-5)
        close(ldj, wl, rtol=1e-5, atol=atol_l)
        close(xr, x, rtol=1e-4, atol=1e-4)
        if n == 300:
            monkeypatch.setenv('STRIBOR_SPLINE_NO_SLAB_FWD', '1')
            n1 = spy['returns']
            ref = flow.log_prob(x.to(DEV), latent=latd)
            monkeypatch.delenv('STRIBOR_SPLINE_NO_SLAB_FWD')
            assert spy['returns'] == n1
            close(lp, ref.cpu(), rtol=1e-5, atol=atol_l)
    st.check_errors()


@pytest.mark.parametrize('hidden,act', [([40, 72], 'Tanh'), ([128, 96], 'ReLU'), ([50], 'ELU')])
def test_wide_slab_forward_behind_deep_conditioners_and_other_activations(hidden, act, spy):
    """_run_spline_slab called directly at K = 20: row-major h of 72 features (guarded loads), of 96 (whole 16-byte pieces), and the
    hidden-layer kernel's fragments over two hidden tiles; scattered transformed columns, a latent input, both directions."""
    torch.manual_seed(len(hidden) * 7 + hidden[-1])
    dim, K, L, mask = 40, 20, 5, 'parity_odd'
    net = st.net.MLP(dim + L, hidden, dim * (3 * K - 1), activation=act)
    cpl = st.Coupling(st.Spline(dim, K, latent_net=net, lower=-2.0, upper=2.0, spline_type='quadratic'), mask=mask)
    lin = net.linears()
    spec = [{'kind': 'coupling_rqs', 'mask': mask, 'n_bins': K, 'lower': -2.0, 'upper': 2.0,
             'net': {'weights': [w.detach().clone() for (w, _) in lin], 'biases': [b.detach().clone() for (_, b) in lin],
                     'activation': act}}]
    spec64 = orc.spec_to(spec, torch.float64)
    cpl = cpl.to(DEV)
    x, lat = torch.randn(777, dim) * 1.4, torch.randn(777, L)
    xd, latd = x.to(DEV), lat.to(DEV)
    for reverse in (True, False):
        y, ldj = cpl._run_spline_slab(xd, latd, reverse, True, 1.0)
        fn = orc.flow_inverse_and_ldj if reverse else orc.flow_forward_and_ldj
        (wy, wl), (wy64, wl64) = fn(spec, x, lat), fn(spec64, x.double(), lat.double())
        _report(f'y reverse={reverse}', y, wy, wy64)
        _report(f'ldj reverse={reverse}', ldj.reshape(-1, 1), wl, wl64)
        close(y, wy, rtol=1e-5, atol=2e-5)
        close(ldj.reshape(-1, 1), wl, rtol=1e-5, atol=2e-4)
    assert spy['returns'] == 2 and spy['entries'].count('sx_rqs_slab_wide_fwd') == 2 and 'sx_rqs_slab_fwd' not in spy['entries']
    st.check_errors()


def _knots(layer, x, K, lower, upper):
    """The layer's width and height knots [n, dim, K + 1] for the rows of x, as the oracle forms them
    (stribor_oracle.rqs_unconstrained: softmax -> cumsum -> pad -> rescale -> pinned ends)."""
    z = orc._conditioning(x, orc._coupling_mask(layer, x), None)
    uw, uh, _ = orc.rqs_params_from_net(orc.mlp_forward(layer['net'], z), x.shape[-1], K)
    out = []
    for u, mn in ((uw, orc.MIN_BIN_WIDTH), (uh, orc.MIN_BIN_HEIGHT)):
        s = mn + (1 - mn * K) * F.softmax(u, dim=-1)
        c = F.pad(torch.cumsum(s, dim=-1), pad=(1, 0), value=0.0)
        c = (upper - lower) * c + lower
        c[..., 0] = lower
        c[..., -1] = upper
        out.append(c)
    return out


@pytest.mark.parametrize('K', [17, 32])
def test_edges_of_the_lane_pair(K, spy):
    """One layer; inputs exactly on the lower bound, the upper bound, knot 16 (the first knot of half 1), knots 15 and 17, and one ulp
    inside and outside each bound -- in the forward direction the width knots, in the inverse the height knots (the spline and its
    derivative are continuous in the knots: whichever neighbouring bin a rounding picks, the values agree within the tier's bounds).
    A NaN input in one row reaches that row only."""
    dim, hidden, lo, hi = 6, 136, -2.5, 2.5
    flow, spec = _flow(dim, hidden, K, ('ordered_right_half',), 0, layers=1, seed=K)
    cpl, layer = flow.transforms[0], spec[0]
    spec64 = orc.spec_to(spec, torch.float64)
    live = (orc.mask_vector('ordered_right_half', dim) <= 0.5).nonzero().flatten()
    base = torch.randn(40, dim) * 1.2
    wk, hk = _knots(layer, base, K, lo, hi)
    f32 = torch.float32
    for reverse in (False, True):
        kn = (hk if reverse else wk)[:, live]                            # [n, n_live, K + 1]; they depend on the conditioning columns only
        points = [kn[..., 0], kn[..., K], kn[..., 16], kn[..., 15], kn[..., min(17, K)],
                  torch.nextafter(torch.tensor(lo, dtype=f32), torch.tensor(0.0)).expand(40, len(live)),
                  torch.nextafter(torch.tensor(lo, dtype=f32), torch.tensor(-9.0)).expand(40, len(live)),
                  torch.nextafter(torch.tensor(hi, dtype=f32), torch.tensor(0.0)).expand(40, len(live)),
                  torch.nextafter(torch.tensor(hi, dtype=f32), torch.tensor(9.0)).expand(40, len(live))]
        assert torch.equal(points[0], torch.full_like(points[0], lo)) and torch.equal(points[1], torch.full_like(points[1], hi))
        xs = []
        for p in points:
            x = base.clone()
            x[:, live] = p
            xs.append(x)
        x = torch.cat(xs)
        fn = orc.flow_inverse_and_ldj if reverse else orc.flow_forward_and_ldj
        (wy, wl), (wy64, wl64) = fn(spec, x), fn(spec64, x.double())
        y, ldj = cpl._run_spline_slab(x.to(DEV), None, reverse, True, 1.0)
        _report(f'y K={K} reverse={reverse}', y, wy, wy64)
        _report(f'ldj K={K} reverse={reverse}', ldj.reshape(-1, 1), wl, wl64)
        close(y, wy, rtol=1e-5, atol=2e-5)
        close(ldj.reshape(-1, 1), wl, rtol=1e-5, atol=2e-4)
        outside = x[:, live].lt(lo) | x[:, live].gt(hi)                  # the linear tails: y = x exactly, no log-det
        assert outside.any() and torch.equal(y.cpu()[:, live][outside], x[:, live][outside])
        # a NaN in a transformed column of one row
        xn = x.clone()
        xn[5, live[1]] = float('nan')
        yn, ln = cpl._run_spline_slab(xn.to(DEV), None, reverse, True, 1.0)
        rest = torch.ones(x.shape[0], dtype=torch.bool)
        rest[5] = False
        assert torch.equal(yn[rest.to(DEV)], y[rest.to(DEV)]) and torch.equal(ln[rest.to(DEV)], ldj[rest.to(DEV)])
        assert torch.isnan(yn[5, live[1]]) and torch.isfinite(yn[5].cpu()[torch.arange(dim) != live[1]]).all()
    assert 'sx_rqs_slab_fwd' not in spy['entries'] and spy['entries'].count('sx_rqs_slab_wide_fwd') == 4
    st.check_errors()


def test_two_calls_return_the_same_bits(spy):
    flow, _ = _flow(64, 160, 24, HALVES, 0, layers=1)
    cpl = flow.transforms[0]
    x = (torch.randn(2049, 64) * 1.5).to(DEV)
    for reverse in (True, False):
        y1, l1 = cpl._run_spline_slab(x, None, reverse, True, 1.0)
        y2, l2 = cpl._run_spline_slab(x, None, reverse, True, 1.0)
        assert torch.equal(y1, y2) and torch.equal(l1, l2)
        assert torch.isfinite(y1).all() and torch.isfinite(l1).all()
    assert spy['entries'].count('sx_rqs_slab_wide_fwd') == 4


def test_log_prob_replays_from_a_hip_graph():
    """test_log_prob_replays_from_a_hip_graph[rqs160] at 24 bins: one capture (a chain of launches, no parallel branches), replayed on
    new input contents, bit-identical to the eager call."""
    dim, n = 64, 1500
    flow, _ = _flow(dim, 160, 24, HALVES, 0, layers=2, seed=11)
    static_x = torch.randn(n, dim, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            flow.log_prob(static_x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static_out = flow.log_prob(static_x)
    for seed in range(2):
        fresh = torch.randn(n, dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * (1 + seed)
        static_x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        got = static_out.clone()
        want = flow.log_prob(fresh)
        assert torch.equal(got, want), seed


def test_neighbours_keep_their_routes(spy):
    """16 bins: sx_rqs_slab_fwd as before.  Cubic splines of 24 bins: the slab tier refuses, the layer-by-layer path answers.
    'exact' arithmetic at 24 bins: no slab entry is called."""
    x = torch.randn(300, 64) * 1.5
    flow, spec = _flow(64, 160, 16, HALVES, 0, layers=2)
    lp = flow.log_prob(x.to(DEV))
    assert spy['returns'] == 2 and spy['entries'].count('sx_rqs_slab_fwd') == 2 and 'sx_rqs_slab_wide_fwd' not in spy['entries']
    close(lp, orc.flow_log_prob(spec, x), rtol=1e-5, atol=4e-4)

    # cubic: the tolerances of test_cubic_spline_couplings_on_the_slab_forward_tier (the same kernels' arithmetic, fp64 oracle)
    flow, spec = _flow(64, 160, 24, HALVES, 0, layers=2, spline_type='cubic')
    spec64 = orc.spec_to(spec, torch.float64)
    del spy['entries'][:]
    lp = flow.log_prob(x.to(DEV))
    y, ldj = flow.forward_and_log_det_jacobian(x.to(DEV))
    assert spy['returns'] == 2 and not any(e in spy['entries'] for e in SLAB_ENTRIES)
    wy, wl = orc.flow_forward_and_ldj(spec64, x.double())
    close(lp, orc.flow_log_prob(spec64, x.double()).float(), rtol=1e-5, atol=1e-4)
    close(y, wy.float(), rtol=1e-5, atol=2e-5)
    close(ldj, wl.float(), rtol=1e-5, atol=1e-4)

    flow, spec = _flow(64, 160, 24, HALVES, 0, layers=2)
    old = st.set_gemm_precision('exact')
    try:
        del spy['entries'][:]
        lp = flow.log_prob(x.to(DEV))
        assert spy['returns'] == 2 and not any(e in spy['entries'] for e in SLAB_ENTRIES)
    finally:
        st.set_gemm_precision(old)
    close(lp, orc.flow_log_prob(spec, x), rtol=1e-5, atol=4e-4)
    st.check_errors()
