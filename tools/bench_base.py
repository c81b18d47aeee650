"""Timing of NormalizingFlow.log_prob under the base densities with parameters, at the shapes of BASELINE cfg 2 (D = 64, 8 affine
couplings) and cfg 3 (D = 64, 8 rational-quadratic spline couplings of 16 bins), --rows rows (default 2^20), bf16 storage.

Lines per shape: UnitNormal (the existing one-launch path), Normal, MultivariateNormal and Uniform (each line says which form the
planner chose: one program -- the base as a trailing step of the flow's program, one launch -- or the flow's inverse pass followed by
one launch of the base's kernel, which for bf16 rows starts with a torch cast of y to fp32), and the baseline of each: the same
build with the equivalent torch.distributions object as `base_dist`, i.e. the fused inverse_and_log_det_jacobian followed by torch ops
on the [n, D] latent (what a user had before these classes).  torch's MultivariateNormal fails at 2^20 rows (its triangular solve's
workspace): that line compares both sides at --mvn-baseline-rows rows, nothing is scaled.

Backward lines: sum(w * Normal.log_prob(x)).backward() with dx, d loc and d scale wanted (sx_base_logprob + sx_normal_logprob_bwd),
D = 8 / 64 / 128, in GB/s of 3 D floats per row (x read twice, dx written once) and against torch autograd of the torch object.

Stand-alone kernels: sx_base_logprob in GB/s of the bytes it must move (x once, 4 B of log-det in and 4 B out per row) against the
8 TB/s HBM peak, fp32 and bf16 rows at D = 64; sx_mvn_logprob in TF of the lower-triangular product it performs (D (D + 1) flops per
row, tiles of 32 rounded up: 2 x 1024 x T (T + 1) / 2) against the 157.3 TF fp32-MFMA peak, at D = 64 and D = 128.

Times are device events around --reps whole calls (launch, output allocation and kernel) after --warmup calls; the rates are the
algorithm's bytes / flops over that call time, not over kernel time.  The build id is recorded with the results.

    python tools/bench_base.py [--rows 1048576] [--reps 100] [--warmup 10] [--mvn-baseline-rows 262144] [--bwd-only] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributions as td

import stribor_amd as st
from stribor_amd.util import flowdesc as fd

PEAK_HBM = 8.0e12
PEAK_F32_MFMA = 157.3e12


def timed(fn, reps, warm):
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


def bases(D, gen):
    loc, scale = torch.randn(D, generator=gen) * 0.1, 0.8 + 0.4 * torch.rand(D, generator=gen)
    tril = torch.tril(torch.randn(D, D, generator=gen) * (0.1 / D ** 0.5), -1) + torch.diag(0.8 + 0.4 * torch.rand(D, generator=gen))
    low, high = torch.full((D,), -60.0), torch.full((D,), 60.0)
    dev = lambda t: t.to('cuda')
    return {
        'UnitNormal': (st.UnitNormal(D), None),
        'Normal': (st.Normal(loc, scale), td.Independent(td.Normal(dev(loc), dev(scale), validate_args=False), 1)),
        'MultivariateNormal': (st.MultivariateNormal(loc, scale_tril=tril), td.MultivariateNormal(dev(loc), scale_tril=dev(tril), validate_args=False)),
        'Uniform': (st.Uniform(low, high), td.Independent(td.Uniform(dev(low), dev(high), validate_args=False), 1)),
    }


def flow_lines(a, results):
    for shape, desc in (('cfg2', fd.cfg2_desc()), ('cfg3', fd.cfg3_desc())):
        gen = torch.Generator().manual_seed(0)
        y = (torch.randn(a.rows, 64, generator=gen) * 0.7).to('cuda').bfloat16()
        for name, (base, torch_base) in bases(64, gen).items():
            torch.manual_seed(0)
            transforms = [fd.build_transform(st, d) for d in desc]
            flow = st.NormalizingFlow(base, transforms).to('cuda')
            with torch.no_grad():
                ms = timed(lambda: flow.log_prob(y), a.reps, a.warmup)
                lp = flow.log_prob(y)
                # (the form is read from the planner, not counted on the device: one program = one library launch; otherwise the
                #  flow's inverse pass and the base's kernel, and for bf16 rows a torch cast of y to fp32 in front of them)
                one = name == 'UnitNormal' or (hasattr(base, '_plan') and flow._base_program(64, 0, y.device) is not None)
                form = 'one program' if one else 'bf16 -> fp32 cast + inverse pass + base kernel'
                r = {'ms': ms, 'rows_per_s': a.rows / ms * 1e3, 'form': form}
                line = f'{shape} {name}: {ms:.3f} ms ({r["rows_per_s"]:.3g} rows/s), {form}'
                if torch_base is not None:
                    baseline = st.NormalizingFlow(torch_base, transforms)
                    # (torch's MultivariateNormal.log_prob runs a library triangular solve whose workspace allocation fails at 2^20
                    #  rows -- HIPBLAS_STATUS_ALLOC_FAILED --: both sides of that comparison are timed at --mvn-baseline-rows, a size
                    #  the library takes; nothing is scaled.  If the library refuses that size too the line says so)
                    small = name == 'MultivariateNormal' and a.rows > a.mvn_baseline_rows
                    yb = y[:a.mvn_baseline_rows] if small else y
                    try:
                        ms_b = timed(lambda: baseline.log_prob(yb), a.reps, a.warmup)
                    except RuntimeError as e:
                        r['torch_base_error'] = str(e)[:200]
                        results[f'{shape}/{name}'] = r
                        print(line + f'; torch.distributions base on the same build: failed at {yb.shape[0]} rows ({str(e)[:80]})')
                        continue
                    ms_same = timed(lambda: flow.log_prob(yb), a.reps, a.warmup) if small else ms
                    diff = (baseline.log_prob(yb) - lp[:yb.shape[0]]).abs().max().item()
                    r.update(torch_base_ms=ms_b, torch_base_rows=yb.shape[0], this_ms_at_those_rows=ms_same, torch_base_over_this=ms_b / ms_same,
                             max_abs_diff=diff)
                    line += (f'; at {yb.shape[0]} rows (torch\'s own triangular solve fails at 2^20): {ms_same:.3f} ms against' if small else ';') + \
                        f' torch.distributions base on the same build {ms_b:.3f} ms = {ms_b / ms_same:.2f} x; max abs difference {diff:.2e}'
            results[f'{shape}/{name}'] = r
            print(line)


def kernel_lines(a, results):
    gen = torch.Generator().manual_seed(1)
    n = a.rows
    for dtype, es in ((torch.float32, 4), (torch.bfloat16, 2)):
        for kind in ('Normal', 'Uniform'):
            d = bases(64, gen)[kind][0].to('cuda')
            x = torch.randn(n, 64, generator=gen).to('cuda').to(dtype)
            ldj = torch.randn(n, generator=gen).to('cuda')
            ms = timed(lambda: d._kernel_rows(x, ldj), 5 * a.reps, a.warmup)          # (tens of microseconds per call)
            gbs = n * (64 * es + 8) / ms / 1e6
            results[f'sx_base_logprob/{kind}/{str(dtype)[6:]}'] = {'ms': ms, 'GBps': gbs, 'frac_of_hbm_peak': gbs * 1e9 / PEAK_HBM}
            print(f'sx_base_logprob {kind} D=64 {str(dtype)[6:]} N={n}: {ms:.3f} ms, {gbs:.0f} GB/s = {gbs * 1e9 / PEAK_HBM:.3f} of the 8 TB/s peak')
    for D in (64, 128):
        d = bases(D, gen)['MultivariateNormal'][0].to('cuda')
        x = torch.randn(n, D, generator=gen).to('cuda')
        ldj = torch.randn(n, generator=gen).to('cuda')
        ms = timed(lambda: d._kernel_rows(x, ldj), 5 * a.reps, a.warmup)          # (tens of microseconds per call)
        T = (D + 31) // 32
        tf = n * 2 * 1024 * T * (T + 1) / 2 / ms / 1e9
        gbs = n * (D * 4 + 8) / ms / 1e6
        results[f'sx_mvn_logprob/D{D}'] = {'ms': ms, 'tflops': tf, 'frac_of_f32_mfma_peak': tf * 1e12 / PEAK_F32_MFMA, 'GBps': gbs}
        print(f'sx_mvn_logprob D={D} fp32 N={n}: {ms:.3f} ms, {tf:.1f} TF = {tf * 1e12 / PEAK_F32_MFMA:.3f} of the fp32-MFMA peak, {gbs:.0f} GB/s')


def backward_lines(a, results):
    """sum(w * Normal.log_prob(x)).backward() with x, loc and scale wanting gradients: sx_base_logprob + sx_normal_logprob_bwd (dx and
    both column sums) against torch autograd of the torch.distributions object; bytes: x read twice, dx written once."""
    gen = torch.Generator().manual_seed(2)
    n = a.rows
    for D in (8, 64, 128):
        loc, scale = torch.randn(D, generator=gen).to('cuda'), (0.8 + 0.4 * torch.rand(D, generator=gen)).to('cuda')
        x = torch.randn(n, D, generator=gen).to('cuda').requires_grad_(True)
        w = torch.randn(n, generator=gen).to('cuda')
        d = st.Normal(torch.nn.Parameter(loc.clone()), torch.nn.Parameter(scale.clone())).to('cuda')
        tl, ts = loc.clone().requires_grad_(True), scale.clone().requires_grad_(True)

        def ours():
            x.grad = d.loc.grad = d.scale.grad = None
            (d.log_prob(x) * w).sum().backward()

        def theirs():
            x.grad = tl.grad = ts.grad = None
            (td.Independent(td.Normal(tl, ts, validate_args=False), 1).log_prob(x) * w).sum().backward()
        ms, ms_t = timed(ours, a.reps, a.warmup), timed(theirs, a.reps, a.warmup)
        gbs = n * (3 * D * 4 + 16) / ms / 1e6
        results[f'normal_fwd_bwd/D{D}'] = {'ms': ms, 'torch_ms': ms_t, 'GBps': gbs, 'frac_of_hbm_peak': gbs * 1e9 / PEAK_HBM}
        print(f'Normal log_prob + backward (dx, d loc, d scale) D={D} N={n}: {ms:.3f} ms, {gbs:.0f} GB/s of algorithmic bytes = '
              f'{gbs * 1e9 / PEAK_HBM:.3f} of the 8 TB/s peak; torch autograd {ms_t:.3f} ms = {ms_t / ms:.2f} x')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--mvn-baseline-rows', type=int, default=1 << 18, help="rows at which the MultivariateNormal line is compared with the torch base (torch's solve fails at 2^20)")
    ap.add_argument('--bwd-only', action='store_true', help='print the backward lines alone')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_base needs a GPU'
    results = {}
    if not a.bwd_only:
        flow_lines(a, results)
        kernel_lines(a, results)
    backward_lines(a, results)
    results['config'] = {'rows': a.rows, 'reps': a.reps, 'warmup': a.warmup, 'storage': 'bf16 (flows)', 'build_id': st._hip.build_id(),
                         'device': torch.cuda.get_device_name(0)}
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
