"""GPU: the second and later trips of a workgroup round the pass loop of the five one-launch CNF kernels (sx_cnf_flow,
sx_cnf_exact_flow, sx_cnf_set_flow, sx_cnf_exact_set_flow, sx_cnf_attn_flow).

The launcher caps the grid at CUs x resident workgroups per CU and every workgroup walks the rest of the batch in a loop; the other
CNF modules stay below a few hundred rows, where no workgroup comes round again.  Here every batch holds at least 2.5 x
passhelp.cap_bound passes (an upper bound of any grid: 256 threads per workgroup against the CU's thread limit), so every workgroup
takes two trips at least and some take one more than others.  The inputs are a short period tiled (77 rows, 7 sets: coprime to the
wave, workgroup and sets-per-pass sizes) and cut so that the last pass is ragged; the outputs are allocated NaN-filled
(passhelp.poison_outputs), so a pass that is skipped or stored at the wrong rows cannot be rescued by what the allocator returns.

  * the four position-invariant kernels: the period alone within cnfhelp.bound (8 x the fp32 sequence's own error against the fp64
    restatement, floor 1e-6 * max(1, max |fp64|)) of the fp64 restatement, then every row i of the big launch bit for bit row
    i % period of that small launch;
  * the attention kernel, whose sums run over the key tiles a wave visits and so depend on a set's slot: every row of the big launch
    within that bound of the period's fp64 values; sets that share slot AND data (one pattern of passes apart) bit for bit; with a
    period of exactly one pass every full pass bit for bit a stand-alone launch of that pass; a NaN set deep in the batch comes back
    non-finite alone."""
import time

import pytest
import torch

import stribor_amd as st

import attnhelp as ah
import cnfhelp as ch
import exacthelp as eh
import exactsethelp as xh
import passhelp as ph
import sethelp as sh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _launch(f, x, lat=None, reverse=False):
    kw = {} if lat is None else {'latent': lat}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        y, l = f.forward_and_log_det_jacobian(x, reverse=reverse, **kw)
    torch.cuda.synchronize()
    assert f._last_path == 'kernel'
    return y, l, (time.perf_counter() - t0) * 1e3


def _check(tag, got, ref, truth):
    tol, e_ref = ch.bound(ref, truth)
    err = (got.cpu().double() - truth).abs().max().item()
    print(f'{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e}')
    assert got.shape == truth.shape
    assert err <= tol, (tag, err, e_ref, tol)


def _check_big(tag, big, ref, truth):
    """Every row of `big` against the period's fp64 values broadcast over it, by _check's rule."""
    tol, e_ref = ch.bound(ref, truth)
    err = ph.max_error(big, truth)
    print(f'{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e} err/e_ref {err / e_ref if e_ref else float("nan"):.2f}')
    assert err <= tol, (tag, err, e_ref, tol)


def _invariant(tag, f, x, lat, refs, truth, reverse, set_size, monkeypatch):
    """Checks (1)-(3) of a position-invariant kernel.  x / lat: the period on the CPU (rows, or sets of `set_size`)."""
    ph.poison_outputs(monkeypatch, DEV)
    n = ph.big_rows(DEV) if set_size == 1 else ph.big_sets(DEV, set_size)
    n_rows = n * set_size
    passes = ph.assert_multi_pass(n_rows, set_size, DEV)
    f = f.to(DEV)
    xd, ld = x.to(DEV), (None if lat is None else lat.to(DEV))
    ys, ls, _ = _launch(f, xd, ld, reverse)
    _check(f'{tag} period y', ys, refs[0], truth[0])
    _check(f'{tag} period ldj', ls, refs[1], truth[1])
    yb, lb, ms = _launch(f, ph.tile(xd, n), None if ld is None else ph.tile(ld, n), reverse)
    print(f'{tag}: cap_bound {ph.cap_bound(DEV)}, {n_rows} rows in {passes} passes, big launch {ms:.1f} ms')
    assert yb.shape[0] == n and lb.shape[:-1] == yb.shape[:-1] and lb.shape[-1] == 1
    ph.assert_tiled(f'{tag} y', yb, ys)
    ph.assert_tiled(f'{tag} ldj', lb, ls)


# ---- sx_cnf_flow ------------------------------------------------------------------------------------------------------------------------
ROW_CASES = {
    # name: (dim, hidden, latent, solver, T with step 0.25, reverse)
    'dim3_latent2_rk4': (3, [16], 2, 'rk4', 0.5, False),
    'dim33_two_tiles_midpoint_reverse': (33, [40, 24], 0, 'midpoint', 0.5, True),
    'dim7_h128x32_trace_from_global_euler3': (7, [128, 32], 0, 'euler', 0.75, False),
}


@pytest.mark.parametrize('name', sorted(ROW_CASES))
def test_rows(name, request, monkeypatch):
    dim, hidden, latent, solver, T, reverse = ROW_CASES[name]
    torch.manual_seed(ph.seed_of(request.node.name))
    g = ph.generator(request.node.name)
    net = st.net.DiffeqMLP(dim + 1 + latent, hidden, dim)
    with torch.no_grad():
        [l for l in net.net.net if isinstance(l, torch.nn.Linear)][-1].bias.normal_()          # (mlp.py:53 zero-fills it)
    f = st.ContinuousTransform(dim, net=net, T=T, divergence='compute', has_latent=latent > 0, solver=solver,
                               solver_options={'step_size': 0.25}).eval()
    x = torch.randn(ph.ROW_PERIOD, dim, generator=g)
    lat = torch.randn(ph.ROW_PERIOD, latent, generator=g) if latent else None
    _invariant(name, f, x, lat, ph.fp32_rows(f, x, lat, reverse), ch.solve64(f, x, lat, reverse=reverse), reverse, 1, monkeypatch)


# ---- sx_cnf_exact_flow ------------------------------------------------------------------------------------------------------------------
EXACT_CASES = {
    # name: (dim, hidden, d_h, latent, solver, T with step 0.25, reverse)
    'one_hidden_latent2_rk4': (5, [32], 3, 2, 'rk4', 0.5, False),
    'two_hidden_euler3_reverse': (4, [24, 16], 2, 0, 'euler', 0.75, True),
}


@pytest.mark.parametrize('name', sorted(EXACT_CASES))
def test_exact_rows(name, request, monkeypatch):
    dim, hidden, d_h, latent, solver, T, reverse = EXACT_CASES[name]
    torch.manual_seed(ph.seed_of(request.node.name))
    g = ph.generator(request.node.name)
    net = st.net.DiffeqExactTraceMLP(dim, hidden, dim, d_h, latent_dim=latent)
    with torch.no_grad():
        net.dimwise_net.net.net[-1].bias.normal_()                                            # (mlp.py:53 zero-fills it)
    f = st.ContinuousTransform(dim, net=net, T=T, divergence='exact', has_latent=latent > 0, solver=solver,
                               solver_options={'step_size': 0.25}).eval()
    x = torch.randn(ph.ROW_PERIOD, dim, generator=g)
    lat = torch.randn(ph.ROW_PERIOD, latent, generator=g) if latent else None
    truth = ch.solve64(f, x, lat, reverse=reverse, func=eh.net64(f.odefunc.diffeq, lat))
    _invariant(name, f, x, lat, ph.fp32_rows(f, x, lat, reverse), truth, reverse, 1, monkeypatch)


# ---- sx_cnf_set_flow --------------------------------------------------------------------------------------------------------------------
SET_CASES = {
    # name: (N, dim, hidden, latent, solver, T with step 0.25, reverse)
    'n5_three_dead_slots_latent2_rk4': (5, 2, [24], 2, 'rk4', 0.5, False),
    'n33_straddles_waves_two_hidden_midpoint': (33, 2, [24, 40], 0, 'midpoint', 0.5, False),
    'n128_one_set_per_pass_euler3_reverse': (128, 2, [16], 0, 'euler', 0.75, True),
}


@pytest.mark.parametrize('name', sorted(SET_CASES))
def test_sets(name, request, monkeypatch):
    N, dim, hidden, latent, solver, T, reverse = SET_CASES[name]
    torch.manual_seed(ph.seed_of(request.node.name))
    g = ph.generator(request.node.name)
    f = sh.make(dim, hidden, latent, T=T, solver=solver, step=0.25)
    with torch.no_grad():
        for l in f.odefunc.diffeq.net.layers:
            l.l1.bias.normal_()
            l.l2.bias.normal_()
    x = torch.randn(ph.SET_PERIOD, N, dim, generator=g)
    lat = torch.randn(ph.SET_PERIOD, N, latent, generator=g) if latent else None
    _invariant(name, f, x, lat, sh.solve32(f, x, lat, reverse=reverse), sh.solve64(f, x, lat, reverse=reverse), reverse, N, monkeypatch)


# ---- sx_cnf_exact_set_flow --------------------------------------------------------------------------------------------------------------
EXACT_SET_CASES = {
    # name: (N, dim, hidden, d_h, latent, pooling, solver, T with step 0.25, reverse)
    'n5_max_latent2_rk4': (5, 3, [16], 3, 2, 'max', 'rk4', 0.5, False),
    'n33_max_two_hidden_midpoint_reverse': (33, 2, [20, 16], 4, 0, 'max', 'midpoint', 0.5, True),
    'n128_mean_euler3': (128, 2, [16], 2, 0, 'mean', 'euler', 0.75, False),
}


@pytest.mark.parametrize('name', sorted(EXACT_SET_CASES))
def test_exact_sets(name, request, monkeypatch):
    N, dim, hidden, d_h, latent, pooling, solver, T, reverse = EXACT_SET_CASES[name]
    g = ph.generator(request.node.name)
    f = xh.make(dim, hidden, d_h, latent=latent, pooling=pooling, T=T, solver=solver, step=0.25, seed=ph.seed_of(request.node.name))
    x = torch.randn(ph.SET_PERIOD, N, dim, generator=g)
    lat = torch.randn(ph.SET_PERIOD, N, latent, generator=g) if latent else None
    _invariant(name, f, x, lat, xh.solve32(f, x, lat, reverse), xh.solve64(f, x, lat, reverse), reverse, N, monkeypatch)


# ---- sx_cnf_attn_flow -------------------------------------------------------------------------------------------------------------------
ATTN_CASES = {
    # name: (N, dim, hidden, heads, mask_diagonal, activation, solver, T with step 0.25, reverse)
    'n5_two_heads_rk4': (5, 2, [12, 8], 2, False, 'Tanh', 'rk4', 0.5, False),
    'n33_mask_diagonal_euler3_odd_evaluations': (33, 2, [8], 2, True, None, 'euler', 0.75, False),
    'n128_two_layer_midpoint_reverse': (128, 2, [24, 16], 4, False, 'ELU', 'midpoint', 0.5, True),
}


def _attn(name, seed_name):
    N, dim, hidden, heads, md, act, solver, T, reverse = ATTN_CASES[name]
    torch.manual_seed(ph.seed_of(seed_name))
    f = ah.make(dim, hidden, n_heads=heads, mask_diagonal=md, T=T, solver=solver, step=0.25, act=act, biases=True)
    return f, N, dim, reverse


@pytest.mark.parametrize('name', sorted(ATTN_CASES))
def test_attention_misaligned_period(name, request, monkeypatch):
    """(b) A period of 7 sets against 25, 3 or 1 sets per pass: every set meets every slot; each row of the big launch within the
    bound of its fp64 values.  Sets one pattern of passes apart (7 passes = 7 x sets-per-pass sets) share slot, neighbours and data:
    those agree bit for bit over the full passes, whichever workgroup took them on whichever trip and exchange area."""
    ph.poison_outputs(monkeypatch, DEV)
    f, N, dim, reverse = _attn(name, request.node.name)
    g = ph.generator(request.node.name)
    x = torch.randn(ph.SET_PERIOD, N, dim, generator=g)
    truth, refs = ah.solve64(f, x, reverse=reverse), ah.solve32(f, x, reverse=reverse)
    n = ph.big_sets(DEV, N)
    passes = ph.assert_multi_pass(n * N, N, DEV)
    f = f.to(DEV)
    xd = x.to(DEV)
    ys, ls, _ = _launch(f, xd, None, reverse)
    _check(f'{name} period y', ys, refs[0], truth[0])
    _check(f'{name} period ldj', ls, refs[1], truth[1])
    yb, lb, ms = _launch(f, ph.tile(xd, n), None, reverse)
    print(f'{name}: cap_bound {ph.cap_bound(DEV)}, {n * N} rows in {passes} passes, big launch {ms:.1f} ms')
    assert yb.shape == (n, N, dim) and lb.shape == (n, N, 1)
    _check_big(f'{name} big y', yb, refs[0], truth[0])
    _check_big(f'{name} big ldj', lb, refs[1], truth[1])
    pattern = ph.SET_PERIOD * (ph.WG_ROWS // N)          # sets after which slot and data repeat together
    full = n - ph.SET_TAIL                                # (the ragged pass visits other key tiles)
    assert full > 2 * pattern
    assert torch.equal(yb[pattern:full], yb[:full - pattern]) and torch.equal(lb[pattern:full], lb[:full - pattern])


_ALIGNED = {}


def _aligned(monkeypatch):
    """The n5 case with a period of exactly one pass (25 sets): the stand-alone launch of the pass and the clean big launch, once."""
    ph.poison_outputs(monkeypatch, DEV)
    if not _ALIGNED:
        name = 'n5_two_heads_rk4'
        f, N, dim, reverse = _attn(name, 'aligned')
        per_pass = ph.WG_ROWS // N
        x = torch.randn(per_pass, N, dim, generator=ph.generator('aligned'))
        truth, refs = ah.solve64(f, x), ah.solve32(f, x)
        n = ph.big_sets(DEV, N)
        f = f.to(DEV)
        xd = x.to(DEV)
        ys, ls, _ = _launch(f, xd)
        xb = ph.tile(xd, n)
        yb, lb, ms = _launch(f, xb)
        print(f'aligned {name}: cap_bound {ph.cap_bound(DEV)}, {n * N} rows in {ph.n_passes(n * N, N)} passes, big launch {ms:.1f} ms')
        _ALIGNED.update(f=f, N=N, n=n, per_pass=per_pass, truth=truth, refs=refs, ys=ys, ls=ls, xb=xb, yb=yb, lb=lb)
    ph.assert_multi_pass(_ALIGNED['n'] * _ALIGNED['N'], _ALIGNED['N'], DEV)
    return _ALIGNED


def test_attention_aligned_period(monkeypatch):
    """(c) The period is one pass of sets: every full pass sees the same data in the same slots and must equal, bit for bit, a
    stand-alone launch of that pass; the ragged last pass (2 sets, other key tiles) stays within the bound."""
    c = _aligned(monkeypatch)
    truth, refs, full = c['truth'], c['refs'], c['n'] - ph.SET_TAIL
    _check('aligned period y', c['ys'], refs[0], truth[0])
    _check('aligned period ldj', c['ls'], refs[1], truth[1])
    assert full % c['per_pass'] == 0
    ph.assert_tiled('aligned y', c['yb'][:full], c['ys'])
    ph.assert_tiled('aligned ldj', c['lb'][:full], c['ls'])
    _check('aligned ragged pass y', c['yb'][full:], refs[0][:ph.SET_TAIL], truth[0][:ph.SET_TAIL])
    _check('aligned ragged pass ldj', c['lb'][full:], refs[1][:ph.SET_TAIL], truth[1][:ph.SET_TAIL])


def test_attention_poisoned_set_deep_in_the_batch(monkeypatch):
    """(d) One set of the aligned batch carries a NaN, more than cap_bound passes into the batch (some workgroup's second or later
    trip): it comes back non-finite in every element, every other row bit for bit as in the clean launch (Tanh embeddings, as
    test_non_finite_sets_stay_alone states it) -- the flags of one trip neither leak into the next nor get lost."""
    c = _aligned(monkeypatch)
    cap = ph.cap_bound(DEV)
    bad = (cap + cap // 2) * c['per_pass'] + 11
    assert bad // c['per_pass'] >= cap and bad < c['n'] - ph.SET_TAIL
    xp = c['xb'].clone()
    xp[bad, 2, 0] = float('nan')
    yp, lp, _ = _launch(c['f'], xp)
    assert not torch.isfinite(yp[bad]).any() and not torch.isfinite(lp[bad]).any()
    for got, clean in ((yp, c['yb']), (lp, c['lb'])):
        assert torch.equal(got[:bad], clean[:bad]) and torch.equal(got[bad + 1:], clean[bad + 1:])
