"""Timing of IResNet on sx_resnet_flow: dim 64, hidden [64, 64], 2^18 rows, the 100-step inverse and the forward, in eval and
training mode, against the composition fallback (product MLP per iteration + torch element-wise ops) on the same shape.

FLOP count: 3 x 2 x 64 x 64 per row and network evaluation (three 64 x 64 layers), so the inverse is 2^18 x 100 x 24576 =
6.4e11 FLOP, 4.1 ms at the 157.3 TF fp32-MFMA peak.  Times are device events around `REPS` calls (each call includes its
sx_spectral_sigma launch; the fallback's own spectral-norm hooks are timed the same way).

    python tools/bench_resnet_flow.py [--rows 262144] [--iterations 100] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 18)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--hidden', type=int, default=64)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_resnet_flow needs a GPU'
    torch.manual_seed(0)
    D, H, N, K = a.dim, a.hidden, a.rows, a.iterations
    f = st.IResNet(D, [H, H]).to('cuda')
    with torch.no_grad():
        for _ in range(5):                       # settle the power iteration (sigma then bounds the Lipschitz constant)
            f(torch.randn(1024, D, device='cuda'))
    y = torch.randn(N, D, device='cuda')
    flop_eval = 2 * (D * H + H * H + H * D)
    results = {}
    with torch.no_grad():
        for mode in ('eval', 'train'):
            f.train(mode == 'train')
            inv = timed(lambda: f.inverse(y, iterations=K), a.reps)
            fwd = timed(lambda: f(y), a.reps)
            fb = timed(lambda: f._composed_reference(y, iterations=K), max(1, a.reps // 5), warm=1)
            fl = N * K * flop_eval
            results[mode] = {'inverse_ms': inv, 'forward_ms': fwd, 'fallback_inverse_ms': fb, 'inverse_rows_per_s': N / inv * 1e3,
                             'forward_rows_per_s': N / fwd * 1e3, 'inverse_tflops': fl / inv / 1e9,
                             'inverse_frac_of_peak': fl / (inv * 1e-3) / PEAK_F32_MFMA, 'fallback_over_kernel': fb / inv}
            r = results[mode]
            print(f'{mode:5s} D={D} H=[{H},{H}] N={N} iterations={K}: inverse {inv:.2f} ms ({r["inverse_rows_per_s"]:.3g} rows/s, '
                  f'{r["inverse_tflops"]:.1f} TF = {r["inverse_frac_of_peak"]:.2f} of the fp32-MFMA peak), forward {fwd:.3f} ms '
                  f'({r["forward_rows_per_s"]:.3g} rows/s); composition fallback inverse {fb:.1f} ms = {r["fallback_over_kernel"]:.1f} x')
        f.eval()
        err = (f.inverse(y, iterations=K) - f._composed_reference(y, iterations=K)).abs().max().item()
        print(f'kernel vs fallback, eval inverse: max abs diff {err:.2e}')
    results['config'] = {'dim': D, 'hidden': [H, H], 'rows': N, 'iterations': K, 'flop_inverse': N * K * flop_eval,
                         'kernel_vs_fallback_max_abs': err}
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
