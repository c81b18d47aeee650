"""CPU: the host side of solver='dopri5_per_sample' -- the specification's fp64 oracle against the truth, the tableau, the constructor
surface, the dispatch, the refusals and the library's entry points."""
import ctypes
import os
import re
from fractions import Fraction as Fr

import pytest
import torch

import adaptivehelp as ah
import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.flows import cnf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_sits_within_a_few_tolerance_units_of_the_tight_solve():
    """At atol = 1e-6, rtol = 1e-5 the oracle's worst row is 3.1 (dim 2 / [64]), 2.1 (dim 5 / [32, 32]) and 4.6 (dim 32 / [64, 64])
    tolerance units from rk4 x 2000 in fp64, measured on the CPU; the bound 10 is 'a few': local error control at tolerance 1 over
    about ten accepted steps."""
    for dim, hidden in ((2, [64]), (5, [32, 32]), (32, [64, 64])):
        f = ah.make(dim, hidden, seed=dim, atol=1e-6, rtol=1e-5)
        x = 1.5 * torch.randn(24, dim)
        o = ah.oracle(f, x)
        ty, tl = ah.tight(f, x)
        u = ah.units(o['y'], o['a'], ty, tl, 1e-6, 1e-5)
        print(dim, hidden, 'worst row, tolerance units:', u.max().item(), 'accepted <=', o['accepted'].max().item())
        assert (o['status'] == 0).all() and u.max().item() <= 10.0


def test_composed_path_takes_the_oracles_decisions_on_decisive_rows():
    """first_step = 0.25, atol = 1e-4, rtol = 1e-3 (the GPU test's setting): where no attempt of the oracle is near a threshold, the fp32
    torch path accepts and rejects as the oracle does, and rejections occur."""
    for dim, hidden in ((2, [64]), (5, [32, 32])):
        f = ah.make(dim, hidden, seed=dim, atol=1e-4, rtol=1e-3, solver_options={'first_step': 0.25})
        x = 1.5 * torch.randn(48, dim)
        o = ah.oracle(f, x, first_step=0.25)
        with torch.no_grad():
            y, l, stats = f._solve_composed_adaptive(x, None, None, False, False)
        dec = o['decisive']
        assert dec.sum() >= 36 and (o['rejected'][dec] > 0).any()
        assert torch.equal(stats[dec, 0].long(), o['accepted'][dec]) and torch.equal(stats[dec, 1].long(), o['rejected'][dec])
        assert (stats[:, 2] == 0).all() and l.shape == (48, 1)
        assert (y.double() - o['y'])[dec].abs().max() < 1e-3 and (l.squeeze(-1).double() - o['a'])[dec].abs().max() < 1e-3


def test_tableau_is_consistent():
    t = cnf.DOPRI5
    exact = lambda v: Fr(v).limit_denominator(10 ** 7)
    assert sum(exact(v) for v in t.b) == 1 and abs(sum(t.e)) < 1e-16
    assert sum(b - s for b, s in zip(ah.B, ah.B_STAR)) == 0 and sum(ah.B) == 1
    for i in range(7):
        assert sum(ah.A[i], Fr(0)) == ah.C[i]
        assert abs(sum(t.a[i]) - t.c[i]) < 1e-15
        assert [float(v) for v in ah.A[i]] == list(t.a[i]) and float(ah.C[i]) == t.c[i]
    assert [float(v) for v in ah.B] == list(t.b) and t.a[6] == t.b[:6]
    assert max(abs(float(v) - w) for v, w in zip(ah.E, t.e)) < 1e-16
    # the kernel's table is the same quotients
    src = open(os.path.join(ROOT, 'stribor_amd', 'csrc', 'sx_cnf_adaptive.hip')).read()
    for frac in ('44.0 / 45.0', '-25360.0 / 2187.0', '46732.0 / 5247.0', '-5103.0 / 18656.0', '5179.0 / 57600.0', '92097.0 / 339200.0'):
        assert frac in src, frac


def test_constructor_and_state_dict_parity_with_an_rk4_twin():
    torch.manual_seed(0)
    a = st.ContinuousTransform(3, net=st.net.DiffeqMLP(4, [16], 3), solver='dopri5_per_sample', atol=1e-7, rtol=1e-4,
                               solver_options={'first_step': 0.1}, test_solver_options={'max_num_steps': 50})
    torch.manual_seed(0)
    b = st.ContinuousTransform(3, net=st.net.DiffeqMLP(4, [16], 3), solver='rk4', solver_options={'step_size': 0.1})
    assert list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    b.load_state_dict(a.state_dict())
    assert (a.atol, a.rtol, a.test_solver) == (1e-7, 1e-4, 'dopri5_per_sample')
    assert a.train()._adaptive_options() == (0.1, cnf.MAX_NUM_STEPS) and a.eval()._adaptive_options() == (None, 50)
    assert a._solver() == ('dopri5_per_sample', None) and a.last_solver_stats is None
    assert cnf.ADAPTIVE_SOLVERS == ('dopri5_per_sample',)
    mixed = st.ContinuousTransform(3, net=st.net.DiffeqMLP(4, [16], 3), solver='rk4', solver_options={'step_size': 0.1},
                                   test_solver='dopri5_per_sample', test_solver_options={})
    assert mixed.train()._solver() == ('rk4', 0.1) and mixed.eval()._solver() == ('dopri5_per_sample', None)


def _route(f, shape, masked=False, graph=False, latent=0):
    return f._choose(torch.Size(shape), latent, masked, graph, True, torch.device('cpu'))


def test_choose_routes_the_new_name():
    f = ah.make(3, [16])
    for want_ldj in (True, False):
        route, plan, trace = f._choose(torch.Size((5, 3)), 0, False, False, want_ldj, torch.device('cpu'))
        assert route == 'sx_cnf_adaptive_flow' and plan is not None and trace == want_ldj
        assert plan[0].trace                                  # the trace is integrated whether or not the caller takes the log-det
    assert _route(ah.make(3, [40, 24], latent=2), (2, 4, 3), latent=2)[0] == 'sx_cnf_adaptive_flow'
    assert _route(ah.make(32, [64, 64]), (5, 32))[0] == 'sx_cnf_adaptive_flow'
    assert _route(ah.make(3, [16], divergence='none'), (5, 3))[:2][0] == 'sx_cnf_adaptive_flow'
    for g, kw in ((ah.make(33, [16]), {}), (ah.make(3, [65]), {}), (ah.make(3, [16, 65]), {}), (f, {'masked': True}), (f, {'graph': True})):
        route, plan, _ = _route(g, (5, g.dim), **kw)
        assert route == 'composed' and plan is None
    assert _route(ah.make(3, [16], set_data=True), (2, 4, 3))[0] == 'composed'
    assert _route(ah.make(3, [16], divergence='compute_set'), (2, 4, 3))[0] == 'composed'
    assert _route(ah.make(3, [16], divergence='approximate').train(), (5, 3))[0] == 'composed'
    torch.manual_seed(0)
    sets = st.ContinuousTransform(3, net=st.net.DiffeqDeepset(4, [16], 3), divergence='compute', set_data=True, solver='dopri5_per_sample').eval()
    assert _route(sets, (2, 4, 3))[0] == 'composed'
    # the same nets under a fixed solver keep their routes
    rk = ah.make(3, [16], solver='rk4', solver_options={'step_size': 0.25})
    assert _route(rk, (5, 3))[0] == 'sx_cnf_flow' and _route(ah.make(3, [65], solver='rk4'), (5, 3))[0] == 'sx_cnf_flow'


def test_other_adaptive_names_still_raise():
    for name in ('dopri5', 'bosh3', 'dopri8', 'adaptive_heun'):
        f = st.ContinuousTransform(2, net=st.net.DiffeqMLP(3, [8], 2), solver=name).eval()
        with pytest.raises(NotImplementedError, match='euler, midpoint, rk4'):
            f._solver()
        with pytest.raises(NotImplementedError, match='dopri5_per_sample'):
            f._grid(False)
    assert st.ContinuousTransform(2, net=st.net.DiffeqMLP(3, [8], 2)).solver == 'dopri5'         # the reference's default stays


def test_unknown_solver_options_raise():
    f = ah.make(2, [8], solver_options={'step_size': 0.1})
    with pytest.raises(NotImplementedError, match='step_size'):
        f._solver()
    with pytest.raises(NotImplementedError, match='step_size'):
        f._solve_composed_adaptive(torch.randn(3, 2), None, None, False, False)
    with pytest.raises(ValueError):
        ah.make(2, [8], solver_options={'first_step': 0.0})._adaptive_options()
    with pytest.raises(ValueError):
        ah.make(2, [8], solver_options={'max_num_steps': 0})._adaptive_options()
    with pytest.raises(ValueError, match='no fixed grid'):
        ah.make(2, [8])._grid(False)


def test_entry_points_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'stribor_hip.h')).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ('sx_cnf_adaptive_lds_bytes', 'sx_cnf_adaptive_flow'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.EXPORTS and hasattr(lib, name), name
    assert 'cnf.py:127-130' in hdr and _hip.lib().sx_abi_version() == 3
    assert 'sx_cnf_adaptive.hip' in open(os.path.join(ROOT, 'stribor_amd', 'csrc', 'Makefile')).read()


def test_planner_sizes_and_argument_validation_without_a_device():
    """sx_cnf_adaptive_lds_bytes answers from the integer fields; sx_cnf_adaptive_flow refuses bad arguments before any launch."""
    f = ah.make(5, [32, 32])
    d, keep = f._adaptive_kernel_net(0, True, torch.device('cpu'))
    lib = _hip.lib()
    assert lib.sx_cnf_adaptive_lds_bytes(d) == 4 * (3 * 1024 + 3 * 32 + 32 + 1024)
    wide = ah.make(5, [65], solver='rk4')._kernel_net(0, True, torch.device('cpu'))[0]
    assert lib.sx_cnf_adaptive_lds_bytes(wide) == 0
    buf = torch.zeros(64)
    stats = torch.zeros(8, 3, dtype=torch.int32)
    call = lambda **k: lib.sx_cnf_adaptive_flow(d, k.get('x', buf.data_ptr()), None, buf.data_ptr(), buf.data_ptr(), k.get('stats', stats.data_ptr()),
                                                k.get('n', 0), 0.0, 1.0, k.get('rtol', 1e-3), k.get('atol', 1e-5), 0.0, k.get('cap', 16), 1, None)
    assert call() == 0                                              # n_rows == 0: validated, nothing launched
    for bad in ({'x': None}, {'stats': None}, {'n': -1}, {'rtol': -1.0}, {'atol': float('nan')}, {'cap': 0}, {'cap': (1 << 20) + 1}):
        assert call(**bad) != 0, bad
    assert lib.sx_cnf_adaptive_flow(wide, buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), stats.data_ptr(), 0, 0.0, 1.0, 1e-3, 1e-5, 0.0, 16, 1, None) != 0
    del keep
