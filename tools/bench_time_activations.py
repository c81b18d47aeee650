"""Timing of the time-dependent point-wise flows (ContinuousTanh / ContinuousActivation): the stand-alone sx_pointwise_time kernel, the
two as steps of the one-launch NeuralFlow program (kernel MODE 21), and the couplings-only NeuralFlow line (kernel MODE 15) of this
build against another build of the library.

Stand-alone, --rows x 64 (default 2^20), fp32 and bf16 rows: ContinuousTanh values only and values + per-element log-derivative, the
tanh and relu mixes (values; they have no log-derivative).  Each line gives the call time, GB/s of the bytes the call must move (x in, y out, the
log-derivative out, 4 B of t per row) and the fraction of the 8 TB/s HBM peak.  Whether a line is bandwidth- or transcendental-bound is
MEASURED against a kernel of another translation unit that moves the same bytes (less the 4 B of t per row) with no per-element
transcendental: sx_pointwise's LeakyReLU, values only or with its log-derivative output.  Within 1.15 x of that time the line is called
bandwidth-bound, beyond it transcendental-bound (the ratio is recorded); the fraction of the HBM peak says how far "bandwidth-bound" is
from the memory system's own limit.  The relu mix is a line of its own: the new kernel with trivial per-element arithmetic.

Mixed NeuralFlow: 4 ContinuousAffineCoupling(MLP(65, [64], 128), TimeTanh) layers (bench.py's NeuralFlow line) with a ContinuousTanh
after each of the first three, D = 64, fp32 rows: forward(x, t) as one launch, and the same module layer by layer on the same build.

Couplings-only NeuralFlow (bench.py's line, kernel MODE 15): --rounds alternating runs of this tree and of the tree at --other-root
(another checkout of the package with its library built, e.g. the parent commit), each run a fresh child process.  Both lists of
timings are recorded, and whether this build's median lies inside the other build's own run-to-run spread (<= its slowest run).

Times are device events around --reps whole calls after --warmup calls.  The build id is recorded with the results.

    python tools/bench_time_activations.py [--rows 1048576] [--reps 50] [--warmup 5] [--other-root DIR] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PEAK_HBM = 8.0e12
BOUND_RATIO = 1.15


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--other-root', default=None, help='another checkout of the package (library built) for the couplings-only comparison')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--root', default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    ap.add_argument('--couplings-only', action='store_true', help=argparse.SUPPRESS)      # (the child process of the comparison)
    return ap.parse_args()


def timed(torch, fn, reps, warm):
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


def couplings(st, torch, n=4, D=64, H=64):
    """bench.py's NeuralFlow layers."""
    return [st.ContinuousAffineCoupling(latent_net=st.net.MLP(D + 1, [H], 2 * D), time_net=st.net.TimeTanh(2 * D),
                                        mask='ordered_0' if i % 2 == 0 else 'ordered_1') for i in range(n)]


def couplings_only(a):
    """Child process: the couplings-only NeuralFlow line of the tree at --root, one JSON line."""
    sys.path.insert(0, a.root)
    import torch
    import stribor_amd as st
    torch.manual_seed(0)
    gen = torch.Generator(device='cuda').manual_seed(0)
    nf = st.NeuralFlow(couplings(st, torch)).to('cuda')
    x = torch.randn(a.rows, 64, device='cuda', generator=gen)
    t = torch.rand(a.rows, 1, device='cuda', generator=gen)
    with torch.no_grad():
        ms = timed(torch, lambda: nf(x, t), a.reps, a.warmup)
    print(json.dumps({'ms': ms, 'build_id': st._hip.build_id(), 'root': os.path.abspath(a.root)}))


def compare(a, results):
    """Alternating child runs: this tree, the other tree, this tree, ...  (the driver has not touched the GPU yet)."""
    runs = {'this': [], 'other': []}
    ids = {}
    for _ in range(a.rounds):
        for who, root in (('this', a.root), ('other', a.other_root)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--couplings-only', '--root', root, '--rows', str(a.rows),
                                  '--reps', str(a.reps), '--warmup', str(a.warmup)], check=True, capture_output=True, text=True, timeout=600)
            r = json.loads(out.stdout.strip().splitlines()[-1])
            runs[who].append(r['ms'])
            ids[who] = r['build_id']
    med = statistics.median(runs['this'])
    inside = med <= max(runs['other'])
    results['neural_flow_couplings_only'] = {'this_ms': runs['this'], 'other_ms': runs['other'], 'this_build_id': ids['this'],
                                             'other_build_id': ids['other'], 'this_median_ms': med,
                                             'other_min_ms': min(runs['other']), 'other_max_ms': max(runs['other']),
                                             'this_median_inside_other_spread': inside}
    print(f'NeuralFlow, 4 time couplings, D=64, N={a.rows} (MODE 15): this build {ids["this"]} ' + ' / '.join(f'{v:.3f}' for v in runs['this']) +
          f' ms; other build {ids["other"]} ' + ' / '.join(f'{v:.3f}' for v in runs['other']) +
          f' ms; this median {med:.3f} ms {"inside" if inside else "OUTSIDE"} the other build\'s spread')


def standalone(a, results, st, torch):
    from stribor_amd import _hip
    from stribor_amd.flows.pointwise import PW_LEAKY, run_pointwise
    from stribor_amd.flows.time_pointwise import run_pointwise_time
    gen = torch.Generator().manual_seed(1)
    n, D = a.rows, 64
    t = (torch.rand(n, generator=gen) * 5).to('cuda')
    for dtype, es in ((torch.float32, 4), (torch.bfloat16, 2)):
        x = (torch.randn(n, D, generator=gen) * 3).to('cuda').to(dtype)
        name = str(dtype)[6:]
        lines = {
            'ContinuousTanh/values': (lambda: run_pointwise_time(x, t, _hip.PWT_TANH_FLOW, 0.0), 2 * es, 'stream/values'),
            'ContinuousTanh/values+ldiag': (lambda: run_pointwise_time(x, t, _hip.PWT_TANH_FLOW, 0.0, want_ldiag=True), 2 * es + 4, 'stream/values+ldiag'),
            'ContinuousTanh/values+ldj': (lambda: run_pointwise_time(x, t, _hip.PWT_TANH_FLOW, 0.0, want_ldj=True), 2 * es, 'stream/values'),
            'ContinuousActivation(tanh)/values': (lambda: run_pointwise_time(x, t, _hip.PWT_MIX_TANH, 1.0), 2 * es, 'stream/values'),
            # (the new kernel with trivial per-element arithmetic: what its per-lane t load, tanh(temperature t) and kind switch cost)
            'ContinuousActivation(relu)/values': (lambda: run_pointwise_time(x, t, _hip.PWT_MIX_RELU, 1.0), 2 * es, 'stream/values'),
        }
        stream = {'stream/values': timed(torch, lambda: run_pointwise(x, PW_LEAKY, 0.1), a.reps, a.warmup),
                  'stream/values+ldiag': timed(torch, lambda: run_pointwise(x, PW_LEAKY, 0.1, want_ldiag=True), a.reps, a.warmup)}
        for k, ms in stream.items():
            per = (2 * es + (4 if 'ldiag' in k else 0))
            gbs = n * D * per / ms / 1e6
            results[f'{k}/{name}'] = {'ms': ms, 'GBps': gbs, 'frac_of_hbm_peak': gbs * 1e9 / PEAK_HBM}
            print(f'{k} (no per-element transcendental) D=64 {name} N={n}: {ms:.3f} ms, {gbs:.0f} GB/s = {gbs * 1e9 / PEAK_HBM:.3f} of the 8 TB/s peak')
        for k, (fn, per, ref) in lines.items():
            ms = timed(torch, fn, a.reps, a.warmup)
            gbs = (n * D * per + 4 * n) / ms / 1e6
            ratio = ms / stream[ref]
            bound = 'bandwidth-bound' if ratio <= BOUND_RATIO else 'transcendental-bound'
            results[f'{k}/{name}'] = {'ms': ms, 'GBps': gbs, 'frac_of_hbm_peak': gbs * 1e9 / PEAK_HBM, 'over_stream_of_same_bytes': ratio, 'bound': bound}
            print(f'{k} D=64 {name} N={n}: {ms:.3f} ms, {gbs:.0f} GB/s = {gbs * 1e9 / PEAK_HBM:.3f} of the 8 TB/s peak; '
                  f'{ratio:.2f} x the stream of the same bytes: {bound}')


def mixed(a, results, st, torch):
    torch.manual_seed(0)
    gen = torch.Generator(device='cuda').manual_seed(0)
    cs = couplings(st, torch)
    layers = [cs[0], st.ContinuousTanh(), cs[1], st.ContinuousTanh(), cs[2], st.ContinuousTanh(), cs[3]]
    nf = st.NeuralFlow(layers).to('cuda')
    x = torch.randn(a.rows, 64, device='cuda', generator=gen)
    t = torch.rand(a.rows, 1, device='cuda', generator=gen)

    def by_layer():
        v = x
        for f in nf.transforms:
            v = f(v, t=t)
        return v
    with torch.no_grad():
        assert nf._fused(64, 0, False, x.device) is not None
        ms = timed(torch, lambda: nf(x, t), a.reps, a.warmup)
        ms_l = timed(torch, by_layer, a.reps, a.warmup)
        diff = (nf(x, t) - by_layer()).abs().max().item()
    results['neural_flow_mixed'] = {'one_launch_ms': ms, 'layer_by_layer_ms': ms_l, 'layer_by_layer_over_one_launch': ms_l / ms,
                                    'rows_per_s': a.rows / ms * 1e3, 'max_abs_diff': diff}
    print(f'NeuralFlow, 4 time couplings + 3 ContinuousTanh, D=64, N={a.rows}: one launch (MODE 21) {ms:.3f} ms ({a.rows / ms * 1e3:.3g} rows/s); '
          f'layer by layer on the same build {ms_l:.3f} ms = {ms_l / ms:.2f} x; max abs difference {diff:.2e}')


def main():
    a = parse()
    if a.couplings_only:
        return couplings_only(a)
    results = {}
    if a.other_root:
        compare(a, results)
    sys.path.insert(0, a.root)
    import torch
    import stribor_amd as st
    assert torch.cuda.is_available(), 'bench_time_activations needs a GPU'
    standalone(a, results, st, torch)
    mixed(a, results, st, torch)
    results['config'] = {'rows': a.rows, 'reps': a.reps, 'warmup': a.warmup, 'build_id': st._hip.build_id(),
                         'device': torch.cuda.get_device_name(0), 'bound_ratio': BOUND_RATIO}
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
