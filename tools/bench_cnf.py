"""Timing of ContinuousTransform on sx_cnf_flow: the log_prob-direction solve (inverse_and_log_det_jacobian: x and the log-det)
at dim 2 / [64] and dim 32 / [128, 128], 2^18 rows, rk4 at 16 steps, against the composition path (the same grid as torch ops,
the divergence by one reverse pass per feature) on the same build.

FLOP count per row and network evaluation: 2 x (dim H1 + H1 H2 + H2 dim) for the forward GEMMs (2 x (dim H + H dim) with one
hidden layer) plus 2 x H2 H1 for the trace GEMM of two hidden layers; 64 evaluations per solve.  The fraction of peak is against
157.3 TF (fp32 MFMA).  Times are device events around `REPS` calls.

The exact-trace line: divergence='exact' over DiffeqExactTraceMLP(8, [64, 64], 8, d_h = 4) on sx_cnf_exact_flow, the same grid and row
count, against its composition path (FuncAndDiagJac: one autograd.grad with a graph per evaluation).  FLOPs per row and evaluation:
the two MADEs 2 x 2 (D H1 + H1 H2 + H2 d_h D), and per dimension the dimwise net 2 (1 + d_h) H1 + 2 H1 H2 + 2 H2 for the value and
2 H1 H2 + 2 H2 for the tangent (the latent-free case; padding to tiles of 32 is not counted).

The set line: set_data=True over DiffeqDeepset(3, [64, 64], 2) on sx_cnf_set_flow, (B, N, dim) = (8192, 32, 2), the same grid, against
its composition path (divergence_exact_for_sets: N x dim reverse passes with a graph per evaluation) timed at --set-fallback-sets sets
and scaled.  FLOPs per element and evaluation: every equivariant layer is two GEMMs (the l1 and l2 branches), 2 x 2 (dim H1 + H1 H2 +
H2 dim), plus five H2 x H1 trace GEMMs, 5 x 2 H2 H1 (padding and the set sums are not counted).

The exact-set line: divergence='exact' over DiffeqExactTraceDeepSet(2, [64, 64], 2, d_h = 4) on sx_cnf_exact_set_flow, the set line's
(B, N, dim) and grid, against its composition path (FuncAndDiagJac) timed at --set-fallback-sets sets and scaled.  FLOPs per element and
evaluation: the MADE and the set embedding 2 (D H1 + H1 H2 + H2 d_h D) + 2 (D H1 + H1 H2 + H2 d_h), and per dimension the dimwise net
as in the exact-trace line (padding and the exchange are not counted).

The attention line: set_data=True / 'compute_set' over DiffeqSelfAttention(3, [64, 32], 2, n_heads=4) on sx_cnf_attn_flow, the set
line's (B, N, dim) and grid, against its composition path (divergence_exact_for_sets through the twice-differentiable attention) timed at
--set-fallback-sets sets and scaled.  FLOPs per element and evaluation: the three embeddings 3 x 2 (dim H1 + H1 E), scores and P.V
2 x 2 N E, the projection 2 E dim, and per coordinate the tangent embeddings 3 x 2 H1 E plus one more score and P.V product 2 x 2 N E
(the recomputed scores, padding and the exchange are not counted).  This line times at least 50 calls (a window over a second), and its
TF / fraction of peak are algorithmic work over CALL time (device events around whole calls: the launch, the output allocation and the
kernel), not over kernel time.  --attention-only prints this line alone.

The exact-attention line: divergence='exact' over DiffeqExactTraceAttention(2, [64, 32], 2, d_h = 4, n_heads = 4) on
sx_cnf_exact_attn_flow, the set line's (B, N, dim) and grid, timed as the attention line (device events around whole calls, at least 50 of
them after 2 warm-up calls), against its composition path (FuncAndDiagJac over the HIP attention core) timed at --set-fallback-sets sets
and scaled, and beside sx_cnf_attn_flow's 'compute_set' call for a DiffeqSelfAttention of the same widths -- what the same user pays for
the trace without the exact-trace construction.  FLOPs per element and evaluation: the q MADE 2 (D H1 + H1 E D), K and V 2 x 2 (D H1 +
H1 E), and per dimension scores and P.V 2 x 2 N E, the projection 2 E d_h and the dimwise net over [H1, E]: 2 (1 + d_h) H1 + 2 H1 E +
2 E for the value and 2 H1 E + 2 E for the tangent (padding and the exchange are not counted).  At the --set-fallback-sets sets it also
checks two conditions and exits non-zero when one fails: the kernel is within 8 x the composition path's own error against an fp64 solve
of the same grid over net.diffeq_exact_trace.closed_form_attn (floor 1e-6 max(1, |fp64|): the tests' bound), and the kernel call is
faster than the composition path.  --exact-attention-only prints this line alone.

The training lines: one step's -log_prob(x).mean().backward() including the zeroing of the gradients, divergence='approximate' in
training mode, at dim 2 / [32] and dim 32 / [32, 32] (the widest hidden layers sx_cnf_train_fwd / sx_cnf_train_bwd cover; dim 2 / [64]
and dim 32 / [64, 64] train on the composition path and are timed on it alone), --train-rows rows, rk4 x --steps: the kernel path, the
composition path on the same build and rows (forced by hiding the kernel plan), and the checkpoint bytes n_steps x rows x dim x 4.
--train-only prints these lines alone.

The adaptive lines: solver='dopri5_per_sample' at the default tolerances (atol 1e-5, rtol 1e-3, automatic first step) on
sx_cnf_adaptive_flow at dim 2 / [64] and dim 32 / [64, 64] (the widest two-layer net that kernel covers), --rows rows, the log_prob
direction: call time (device events around whole calls), the composed adaptive path on the same build timed at --fallback-rows rows and
scaled, the mean and the largest number of attempts per row (last_solver_stats), and sx_cnf_flow's rk4 x --steps on the same net and
rows for scale.  --adaptive-only prints these lines alone.

    python tools/bench_cnf.py [--rows 262144] [--steps 16] [--json out.json] [--attention-only] [--exact-attention-only] [--train-only] [--train-rows 16384] [--adaptive-only]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import stribor_amd as st

PEAK_F32_MFMA = 157.3e12


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def attention_line(a, results):
    torch.manual_seed(0)
    B, N, D, hidden, heads = a.sets, 32, 2, [64, 32], 4
    f = st.ContinuousTransform(D, net=st.net.DiffeqSelfAttention(D + 1, hidden, D, n_heads=heads), divergence='compute_set', solver='rk4',
                               solver_options={'step_size': 1.0 / a.steps}, set_data=True).eval().to('cuda')
    y = torch.randn(B, N, D, device='cuda')
    ys = y[:a.set_fallback_sets]
    H1, E = hidden
    flop_eval = 6 * (D * H1 + H1 * E) + 4 * N * E + 2 * E * D + D * (6 * H1 * E + 4 * N * E)
    reps = max(a.reps, 50)                 # (a call takes tens of ms: at least 50 of them, so that the timed window is over a second)
    with torch.no_grad():
        ms = timed(lambda: f.inverse_and_log_det_jacobian(y), reps)
        assert f._last_path == 'kernel'
        ms_x = timed(lambda: f.inverse(y), reps)
        fb = timed(lambda: f._composed_reference(ys, reverse=True), 1, warm=0) * (B / ys.shape[0])
        xk, lk = f.inverse_and_log_det_jacobian(ys)
        xc, lc = f._composed_reference(ys, reverse=True)
    fl = B * N * 4 * a.steps * flop_eval
    r = results[f'attention_b{B}_n{N}_dim{D}_h{"x".join(map(str, hidden))}_heads{heads}'] = {
        'solve_ldj_ms': ms, 'solve_only_ms': ms_x, 'composed_ms_scaled': fb, 'rows_per_s': B * N / ms * 1e3, 'tflops': fl / ms / 1e9,
        'frac_of_peak': fl / (ms * 1e-3) / PEAK_F32_MFMA, 'composed_over_kernel': fb / ms, 'reps': reps,
        'max_abs_x': (xk - xc).abs().max().item(), 'max_abs_ldj': (lk - lc).abs().max().item()}
    print(f'attention sets (B, N, dim) = ({B}, {N}, {D}) {hidden} heads {heads} rk4 x {a.steps}: solve + log-det {ms:.2f} ms '
          f'per call over {reps} calls ({r["rows_per_s"]:.3g} elements/s, {r["tflops"]:.1f} TF of algorithmic work per call time = '
          f'{r["frac_of_peak"]:.3f} of the fp32-MFMA peak), solve alone {ms_x:.2f} ms; composition path {fb:.0f} ms (timed at '
          f'{ys.shape[0]} sets, scaled) = {r["composed_over_kernel"]:.0f} x; kernel vs composition max abs x {r["max_abs_x"]:.2e} ldj '
          f'{r["max_abs_ldj"]:.2e}')


def exact_attention_line(a, results):
    from stribor_amd.flows.cnf import _rk_step
    from stribor_amd.net import diffeq_exact_trace as xt
    from stribor_amd.net.diffeq_exact_trace import closed_form_attn
    torch.manual_seed(0)
    B, N, D, hidden, d_h, heads = a.sets, 32, 2, [64, 32], 4, 4
    opts = dict(solver='rk4', solver_options={'step_size': 1.0 / a.steps})
    f = st.ContinuousTransform(D, net=xt.DiffeqExactTraceAttention(D, hidden, D, d_h, n_heads=heads), divergence='exact',
                               **opts).eval().to('cuda')
    same_width = st.ContinuousTransform(D, net=st.net.DiffeqSelfAttention(D + 1, hidden, D, n_heads=heads), divergence='compute_set',
                                        set_data=True, **opts).eval().to('cuda')
    y = torch.randn(B, N, D, device='cuda')
    ys = y[:a.set_fallback_sets]
    H1, E = hidden
    flop_eval = 2 * (D * H1 + H1 * E * D) + 4 * (D * H1 + H1 * E) + D * (4 * N * E + 2 * E * d_h + 2 * (1 + d_h) * H1 + 4 * H1 * E + 4 * E)
    reps = max(a.reps, 50)

    def solve64(x):
        """The same grid and tableau (flows.cnf._rk_step) over the closed form in fp64 -> (x at 0, log-det)."""
        net = f.odefunc.diffeq

        def func(t, state):
            dy, jac = closed_form_attn(net, float(t), state[0], dtype=torch.float64)
            return dy, -jac
        grid = f._grid(True).points
        state = (x.double(), torch.zeros_like(x, dtype=torch.float64))
        for i in range(len(grid) - 1):
            state = tuple(s + d for s, d in zip(state, _rk_step(func, 'rk4', grid[i], grid[i + 1], state)))
        return state[0], -state[1].sum(-1, keepdim=True)
    with torch.no_grad():
        ms = timed(lambda: f.inverse_and_log_det_jacobian(y), reps)
        assert f._last_path == 'kernel'
        ms_x = timed(lambda: f.inverse(y), reps)
        ms_cs = timed(lambda: same_width.inverse_and_log_det_jacobian(y), reps)
        assert same_width._last_path == 'kernel'
        ms_small = timed(lambda: f.inverse_and_log_det_jacobian(ys), reps)
        fb_small = timed(lambda: f._composed_reference(ys, reverse=True), 1, warm=1)
        fb = fb_small * (B / ys.shape[0])
        xk, lk = f.inverse_and_log_det_jacobian(ys)
        xc, lc = f._composed_reference(ys, reverse=True)
        x64, l64 = solve64(ys)
    bound = lambda ref32, truth: max(8 * (ref32.double() - truth).abs().max().item(), 1e-6 * max(1.0, truth.abs().max().item()))
    err_x, err_l = (xk.double() - x64).abs().max().item(), (lk.double() - l64).abs().max().item()
    bound_x, bound_l = bound(xc, x64), bound(lc, l64)
    fl = B * N * 4 * a.steps * flop_eval
    r = results[f'exact_attention_b{B}_n{N}_dim{D}_dh{d_h}_h{"x".join(map(str, hidden))}_heads{heads}'] = {
        'solve_ldj_ms': ms, 'solve_only_ms': ms_x, 'composed_ms_scaled': fb, 'rows_per_s': B * N / ms * 1e3, 'tflops': fl / ms / 1e9,
        'frac_of_peak': fl / (ms * 1e-3) / PEAK_F32_MFMA, 'composed_over_kernel': fb / ms, 'reps': reps,
        'compute_set_same_width_ms': ms_cs, 'compute_set_over_exact': ms_cs / ms,
        'sets_small': ys.shape[0], 'kernel_small_ms': ms_small, 'composed_small_ms': fb_small, 'kernel_faster_at_small': ms_small < fb_small,
        'max_abs_x': (xk - xc).abs().max().item(), 'max_abs_ldj': (lk - lc).abs().max().item(),
        'kernel_err_x_vs_fp64': err_x, 'bound_x': bound_x, 'kernel_err_ldj_vs_fp64': err_l, 'bound_ldj': bound_l,
        'within_bound': err_x <= bound_x and err_l <= bound_l}
    print(f'exact-trace attention sets (B, N, dim) = ({B}, {N}, {D}) d_h {d_h} {hidden} heads {heads} rk4 x {a.steps}: solve + log-det '
          f'{ms:.2f} ms per call over {reps} calls ({r["rows_per_s"]:.3g} elements/s, {r["tflops"]:.1f} TF of algorithmic work per call '
          f'time = {r["frac_of_peak"]:.3f} of the fp32-MFMA peak), solve alone {ms_x:.2f} ms; composition path {fb:.0f} ms (timed at '
          f'{ys.shape[0]} sets: {fb_small:.1f} ms against the kernel\'s {ms_small:.3f} ms there, scaled) = {r["composed_over_kernel"]:.0f} x; '
          f'kernel vs composition max abs x {r["max_abs_x"]:.2e} ldj {r["max_abs_ldj"]:.2e}; kernel vs fp64 x {err_x:.2e} (bound '
          f'{bound_x:.2e}) ldj {err_l:.2e} (bound {bound_l:.2e}); sx_cnf_attn_flow under compute_set at the same widths {ms_cs:.2f} ms = '
          f'{r["compute_set_over_exact"]:.2f} x this call')
    return r['within_bound'] and r['kernel_faster_at_small']


def training_lines(a, results):
    n = a.train_rows
    for dim, hidden in ((2, [32]), (32, [32, 32]), (2, [64]), (32, [64, 64])):
        torch.manual_seed(0)
        cnf = st.ContinuousTransform(dim, net=st.net.DiffeqMLP(dim + 1, hidden, dim), divergence='approximate', solver='rk4',
                                     solver_options={'step_size': 1.0 / a.steps})
        flow = st.NormalizingFlow(st.UnitNormal(dim), [cnf]).to('cuda').train()
        x = torch.randn(n, dim, device='cuda')

        def step():
            flow.zero_grad(set_to_none=True)
            (-flow.log_prob(x).mean()).backward()
        covered = cnf._train_kernel_net(0, x.device) is not None
        ms = timed(step, a.reps) if covered else None
        assert not covered or cnf._last_path == 'kernel'
        plan = cnf._train_kernel_net
        cnf._train_kernel_net = lambda *args: None          # (the composition path on the same build)
        fb = timed(step, max(1, a.reps // 2), warm=1)
        assert cnf._last_path == 'composed'
        cnf._train_kernel_net = plan
        ckpt = a.steps * n * dim * 4
        key = f'train_dim{dim}_h{"x".join(map(str, hidden))}'
        results[key] = {'rows': n, 'kernel_step_ms': ms, 'composed_step_ms': fb, 'composed_over_kernel': (fb / ms if covered else None),
                        'checkpoint_bytes': ckpt if covered else 0}
        if covered:
            print(f'training dim {dim} {hidden} N={n} rk4 x {a.steps}: kernel path {ms:.2f} ms per step, composition path {fb:.1f} ms '
                  f'= {fb / ms:.1f} x; checkpoints {ckpt} bytes')
        else:
            print(f'training dim {dim} {hidden} N={n} rk4 x {a.steps}: outside the training kernels (hidden > 32), composition path '
                  f'{fb:.1f} ms per step')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 18)
    ap.add_argument('--fallback-rows', type=int, default=1 << 14, help='rows of the composition-path timing (scaled to --rows)')
    ap.add_argument('--sets', type=int, default=8192, help='B of the set line (N = 32, dim = 2)')
    ap.add_argument('--set-fallback-sets', type=int, default=64, help="sets of the set line's composition-path timing (scaled to --sets)")
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--attention-only', action='store_true', help='print the attention line alone')
    ap.add_argument('--exact-attention-only', action='store_true', help='print the exact-trace attention line alone')
    ap.add_argument('--train-only', action='store_true', help='print the training lines alone')
    ap.add_argument('--adaptive-only', action='store_true', help="print the 'dopri5_per_sample' lines alone")
    ap.add_argument('--train-rows', type=int, default=1 << 14, help='rows of the training lines (the composition path finishes in seconds)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_cnf needs a GPU'
    results = {}
    only = a.attention_only or a.exact_attention_only or a.train_only or a.adaptive_only
    ok = True
    if not only:
        earlier_lines(a, results)
    if a.attention_only or not only:
        attention_line(a, results)
    if a.exact_attention_only or not only:
        ok = exact_attention_line(a, results)
    if a.train_only or not only:
        training_lines(a, results)
    if a.adaptive_only or not only:
        adaptive_lines(a, results)
    results['config'] = {'rows': a.rows, 'steps': a.steps, 'solver': 'rk4', 'fallback_rows': a.fallback_rows, 'sets': a.sets,
                         'set_fallback_sets': a.set_fallback_sets, 'train_rows': a.train_rows,
                         'build_id': st._hip.build_id()}
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(results, fh, indent=1)
    if not ok:
        sys.exit('bench_cnf: the exact-attention line misses one of its two conditions (within_bound, kernel_faster_at_small)')


def adaptive_lines(a, results):
    for dim, hidden in ((2, [64]), (32, [64, 64])):
        torch.manual_seed(0)
        net = st.net.DiffeqMLP(dim + 1, hidden, dim)
        f = st.ContinuousTransform(dim, net=net, divergence='compute', solver='dopri5_per_sample').eval().to('cuda')
        fixed = st.ContinuousTransform(dim, net=net, divergence='compute', solver='rk4', solver_options={'step_size': 1.0 / a.steps}).eval().to('cuda')
        y = torch.randn(a.rows, dim, device='cuda')
        ys = y[:a.fallback_rows]
        with torch.no_grad():
            ms = timed(lambda: f.inverse_and_log_det_jacobian(y), a.reps)
            assert f._last_path == 'kernel'
            stats = f.last_solver_stats
            attempts = stats[:, :2].sum(-1).float()
            failed = int((stats[:, 2] != 0).sum().item())
            num_evals = f._num_evals()                 # (read now: the composed reference below resets the counter)
            ms_rk4 = timed(lambda: fixed.inverse_and_log_det_jacobian(y), a.reps)
            assert fixed._last_path == 'kernel'
            fb = timed(lambda: f._composed_reference(ys, reverse=True), 1, warm=1) * (a.rows / ys.shape[0])
            xk, lk = f.inverse_and_log_det_jacobian(ys)
            xc, lc = f._composed_reference(ys, reverse=True)
        r = results[f'adaptive_dim{dim}_h{"x".join(map(str, hidden))}'] = {
            'solve_ldj_ms': ms, 'composed_ms_scaled': fb, 'composed_over_kernel': fb / ms, 'rows_per_s': a.rows / ms * 1e3,
            'attempts_mean': attempts.mean().item(), 'attempts_max': int(attempts.max().item()), 'rejected': int(stats[:, 1].sum().item()),
            'failed_rows': failed, 'num_evals': num_evals, 'rk4_ms': ms_rk4, 'rk4_steps': a.steps, 'atol': f.atol, 'rtol': f.rtol,
            'max_abs_x': (xk - xc).abs().max().item(), 'max_abs_ldj': (lk - lc).abs().max().item()}
        print(f'adaptive dim {dim} {hidden} N={a.rows} dopri5_per_sample atol {f.atol:g} rtol {f.rtol:g}: solve + log-det {ms:.2f} ms per call '
              f'({r["rows_per_s"]:.3g} rows/s), attempts per row mean {r["attempts_mean"]:.2f} max {r["attempts_max"]} ({r["rejected"]} rejected, '
              f'{failed} failed rows); composed adaptive path {fb:.0f} ms (timed at {ys.shape[0]} rows, scaled) = {r["composed_over_kernel"]:.0f} x; '
              f'sx_cnf_flow rk4 x {a.steps} on the same net {ms_rk4:.2f} ms; kernel vs composed max abs x {r["max_abs_x"]:.2e} ldj {r["max_abs_ldj"]:.2e}')


def earlier_lines(a, results):
    for dim, hidden in ((2, [64]), (32, [128, 128])):
        torch.manual_seed(0)
        f = st.ContinuousTransform(dim, net=st.net.DiffeqMLP(dim + 1, hidden, dim), divergence='compute', solver='rk4',
                                   solver_options={'step_size': 1.0 / a.steps}).eval().to('cuda')
        y = torch.randn(a.rows, dim, device='cuda')
        ys = y[:a.fallback_rows]
        widths = [dim] + hidden + [dim]
        flop_eval = 2 * sum(p * q for p, q in zip(widths[:-1], widths[1:])) + (2 * hidden[0] * hidden[1] if len(hidden) == 2 else 0)
        evals = 4 * a.steps
        with torch.no_grad():
            ms = timed(lambda: f.inverse_and_log_det_jacobian(y), a.reps)
            assert f._last_path == 'kernel'
            ms_x = timed(lambda: f.inverse(y), a.reps)
            fb = timed(lambda: f._composed_reference(ys, reverse=True), 1, warm=1) * (a.rows / ys.shape[0])
            xk, lk = f.inverse_and_log_det_jacobian(ys)
            xc, lc = f._composed_reference(ys, reverse=True)
        fl = a.rows * evals * flop_eval
        key = f'dim{dim}_h{"x".join(map(str, hidden))}'
        results[key] = {'solve_ldj_ms': ms, 'solve_only_ms': ms_x, 'composed_ms_scaled': fb, 'rows_per_s': a.rows / ms * 1e3,
                        'tflops': fl / ms / 1e9, 'frac_of_peak': fl / (ms * 1e-3) / PEAK_F32_MFMA, 'composed_over_kernel': fb / ms,
                        'max_abs_x': (xk - xc).abs().max().item(), 'max_abs_ldj': (lk - lc).abs().max().item()}
        r = results[key]
        print(f'dim {dim} {hidden} N={a.rows} rk4 x {a.steps}: solve + log-det {ms:.2f} ms ({r["rows_per_s"]:.3g} rows/s, '
              f'{r["tflops"]:.1f} TF = {r["frac_of_peak"]:.3f} of the fp32-MFMA peak), solve alone {ms_x:.2f} ms; composition path '
              f'{fb:.0f} ms (timed at {ys.shape[0]} rows, scaled) = {r["composed_over_kernel"]:.0f} x; kernel vs composition max abs '
              f'x {r["max_abs_x"]:.2e} ldj {r["max_abs_ldj"]:.2e}')
    # the exact-trace net
    torch.manual_seed(0)
    D, d_h, hidden = 8, 4, [64, 64]
    f = st.ContinuousTransform(D, net=st.net.DiffeqExactTraceMLP(D, hidden, D, d_h), divergence='exact', solver='rk4',
                               solver_options={'step_size': 1.0 / a.steps}).eval().to('cuda')
    y = torch.randn(a.rows, D, device='cuda')
    ys = y[:a.fallback_rows]
    H1, H2 = hidden
    flop_eval = 4 * (D * H1 + H1 * H2 + H2 * d_h * D) + D * (2 * (1 + d_h) * H1 + 4 * H1 * H2 + 4 * H2)
    with torch.no_grad():
        ms = timed(lambda: f.inverse_and_log_det_jacobian(y), a.reps)
        assert f._last_path == 'kernel'
        ms_x = timed(lambda: f.inverse(y), a.reps)
        fb = timed(lambda: f._composed_reference(ys, reverse=True), 1, warm=1) * (a.rows / ys.shape[0])
        xk, lk = f.inverse_and_log_det_jacobian(ys)
        xc, lc = f._composed_reference(ys, reverse=True)
    fl = a.rows * 4 * a.steps * flop_eval
    r = results[f'exact_dim{D}_dh{d_h}_h{"x".join(map(str, hidden))}'] = {
        'solve_ldj_ms': ms, 'solve_only_ms': ms_x, 'composed_ms_scaled': fb, 'rows_per_s': a.rows / ms * 1e3, 'tflops': fl / ms / 1e9,
        'frac_of_peak': fl / (ms * 1e-3) / PEAK_F32_MFMA, 'composed_over_kernel': fb / ms,
        'max_abs_x': (xk - xc).abs().max().item(), 'max_abs_ldj': (lk - lc).abs().max().item()}
    print(f'exact trace dim {D} d_h {d_h} {hidden} N={a.rows} rk4 x {a.steps}: solve + log-det {ms:.2f} ms ({r["rows_per_s"]:.3g} rows/s, '
          f'{r["tflops"]:.1f} TF = {r["frac_of_peak"]:.3f} of the fp32-MFMA peak), solve alone {ms_x:.2f} ms; composition path '
          f'{fb:.0f} ms (timed at {ys.shape[0]} rows, scaled) = {r["composed_over_kernel"]:.1f} x; kernel vs composition max abs '
          f'x {r["max_abs_x"]:.2e} ldj {r["max_abs_ldj"]:.2e}')
    # the set net
    torch.manual_seed(0)
    B, N, D, hidden = a.sets, 32, 2, [64, 64]
    f = st.ContinuousTransform(D, net=st.net.DiffeqDeepset(D + 1, hidden, D), divergence='compute', solver='rk4',
                               solver_options={'step_size': 1.0 / a.steps}, set_data=True).eval().to('cuda')
    y = torch.randn(B, N, D, device='cuda')
    ys = y[:a.set_fallback_sets]
    H1, H2 = hidden
    flop_eval = 4 * (D * H1 + H1 * H2 + H2 * D) + 10 * H2 * H1
    with torch.no_grad():
        ms = timed(lambda: f.inverse_and_log_det_jacobian(y), a.reps)
        assert f._last_path == 'kernel'
        ms_x = timed(lambda: f.inverse(y), a.reps)
        fb = timed(lambda: f._composed_reference(ys, reverse=True), 1, warm=0) * (B / ys.shape[0])
        xk, lk = f.inverse_and_log_det_jacobian(ys)
        xc, lc = f._composed_reference(ys, reverse=True)
    fl = B * N * 4 * a.steps * flop_eval
    r = results[f'set_b{B}_n{N}_dim{D}_h{"x".join(map(str, hidden))}'] = {
        'solve_ldj_ms': ms, 'solve_only_ms': ms_x, 'composed_ms_scaled': fb, 'rows_per_s': B * N / ms * 1e3, 'tflops': fl / ms / 1e9,
        'frac_of_peak': fl / (ms * 1e-3) / PEAK_F32_MFMA, 'composed_over_kernel': fb / ms,
        'max_abs_x': (xk - xc).abs().max().item(), 'max_abs_ldj': (lk - lc).abs().max().item()}
    print(f'sets (B, N, dim) = ({B}, {N}, {D}) {hidden} rk4 x {a.steps}: solve + log-det {ms:.2f} ms ({r["rows_per_s"]:.3g} elements/s, '
          f'{r["tflops"]:.1f} TF = {r["frac_of_peak"]:.3f} of the fp32-MFMA peak), solve alone {ms_x:.2f} ms; composition path '
          f'{fb:.0f} ms (timed at {ys.shape[0]} sets, scaled) = {r["composed_over_kernel"]:.0f} x; kernel vs composition max abs '
          f'x {r["max_abs_x"]:.2e} ldj {r["max_abs_ldj"]:.2e}')
    # the exact-trace set net
    torch.manual_seed(0)
    d_h = 4
    f = st.ContinuousTransform(D, net=st.net.DiffeqExactTraceDeepSet(D, hidden, D, d_h), divergence='exact', solver='rk4',
                               solver_options={'step_size': 1.0 / a.steps}).eval().to('cuda')
    flop_eval = 2 * (D * H1 + H1 * H2 + H2 * d_h * D) + 2 * (D * H1 + H1 * H2 + H2 * d_h) + D * (2 * (1 + d_h) * H1 + 4 * H1 * H2 + 4 * H2)
    with torch.no_grad():
        ms = timed(lambda: f.inverse_and_log_det_jacobian(y), a.reps)
        assert f._last_path == 'kernel'
        ms_x = timed(lambda: f.inverse(y), a.reps)
        fb = timed(lambda: f._composed_reference(ys, reverse=True), 1, warm=1) * (B / ys.shape[0])
        xk, lk = f.inverse_and_log_det_jacobian(ys)
        xc, lc = f._composed_reference(ys, reverse=True)
    fl = B * N * 4 * a.steps * flop_eval
    r = results[f'exact_set_b{B}_n{N}_dim{D}_dh{d_h}_h{"x".join(map(str, hidden))}'] = {
        'solve_ldj_ms': ms, 'solve_only_ms': ms_x, 'composed_ms_scaled': fb, 'rows_per_s': B * N / ms * 1e3, 'tflops': fl / ms / 1e9,
        'frac_of_peak': fl / (ms * 1e-3) / PEAK_F32_MFMA, 'composed_over_kernel': fb / ms,
        'max_abs_x': (xk - xc).abs().max().item(), 'max_abs_ldj': (lk - lc).abs().max().item()}
    print(f'exact-trace sets (B, N, dim) = ({B}, {N}, {D}) d_h {d_h} {hidden} rk4 x {a.steps}: solve + log-det {ms:.2f} ms '
          f'({r["rows_per_s"]:.3g} elements/s, {r["tflops"]:.1f} TF = {r["frac_of_peak"]:.3f} of the fp32-MFMA peak), solve alone '
          f'{ms_x:.2f} ms; composition path {fb:.0f} ms (timed at {ys.shape[0]} sets, scaled) = {r["composed_over_kernel"]:.1f} x; kernel '
          f'vs composition max abs x {r["max_abs_x"]:.2e} ldj {r["max_abs_ldj"]:.2e}')


if __name__ == '__main__':
    main()
