"""Timing of NeuralFlow TRAINING on sx_time_coupling_bwd: the README's NeuralFlow line (4 x ContinuousAffineCoupling, TimeTanh,
dim 64, hidden 64, masks alternating) at 2^18 rows.  Three cases, device events around `--reps` steps:

    (a) f(x, t) + backward          (b) one Adam step (zero_grad, forward, loss, backward, update)
    (c) the backward call of ONE stand-alone layer alone (sx_time_coupling_bwd: its kernel and the ordered sum), with its share of
        the fp32-MFMA peak and of the HBM bandwidth

(a) and (b) run on the kernel path and on the composition path of the same build (the planner `_train_plan` patched to None, which
is `_run_composed`, the parent commit's code), in `--runs` alternating runs of one warm-up step and `--reps` timed steps each, the same
for both paths; the figures are the median and the spread (max - min) over the runs.  On a build without the kernel path (no
`_train_plan`) only the composition path is timed: run the tool from a checkout of the parent commit with --json, then pass that file
to this build's run as --merge-parent, which copies its cases into the result as `parent_commit`.

What (c) needs, from the shapes: per row the pruned conditioner forward, its two transpose products and its two contractions,
6 (K H + 2 n_live H) FLOP with K conditioning inputs; x, gy and gx (dim floats each) and t, gl, gt of HBM traffic.
The recompute's transcendentals and the kernel's partial-buffer traffic are not counted, so the two shares of peak it prints are
lower bounds on the utilisation.

    python tools/bench_neural_flow_train.py [--rows 262144] [--json profiles/neural_flow_train_bench.json] [--merge-parent parent_run.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.flows.coupling import ContinuousAffineCoupling

PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12


def timed(fn, reps, warm=1):
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


class Composed:
    """Inside: every ContinuousAffineCoupling under `module` takes the composition path."""

    def __init__(self, module):
        self.mods = [m for m in module.modules() if hasattr(m, '_train_plan')]

    def __enter__(self):
        for m in self.mods:
            m._train_plan = lambda *a: None

    def __exit__(self, *exc):
        for m in self.mods:
            del m._train_plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 18)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--hidden', type=int, default=64)
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--merge-parent', default=None, help="a --json result of this tool run on the parent commit's checkout")
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_neural_flow_train needs a GPU'
    torch.manual_seed(0)
    D, H, N = a.dim, a.hidden, a.rows

    def layer(i):
        mask = 'ordered_left_half' if i % 2 == 0 else 'ordered_right_half'
        return st.ContinuousAffineCoupling(st.net.MLP(D + 1, [H], 2 * D), st.net.TimeTanh(2 * D), mask)

    f = layer(0).to('cuda')
    nf = st.NeuralFlow([layer(i) for i in range(a.layers)]).to('cuda')
    opt = torch.optim.Adam(nf.parameters(), lr=1e-4)
    has_kernel = hasattr(ContinuousAffineCoupling, '_train_plan')
    x = torch.randn(N, D, device='cuda', requires_grad=True)
    t = torch.rand(N, 1, device='cuda')
    cot = torch.randn(N, D, device='cuda')
    target = torch.randn(N, D, device='cuda')

    def step_a():
        nf.zero_grad(set_to_none=True)
        x.grad = None
        nf(x, t=t).backward(cot)

    def step_b():
        opt.zero_grad(set_to_none=True)
        x.grad = None
        (nf(x, t=t) - target).square().mean().backward()
        opt.step()

    cases = {'a_forward_backward': step_a, 'b_adam_step': step_b}
    raw = {name: {'kernel': [], 'composed': []} for name in cases}
    for _ in range(a.runs):                      # alternating runs: kernel, composed, kernel, ...
        for name, step in cases.items():
            if has_kernel:
                raw[name]['kernel'].append(timed(step, a.reps))
                assert all(m._last_path == 'kernel' for m in nf.transforms)
            with Composed(nf):
                raw[name]['composed'].append(timed(step, a.reps))
    results = {'build_id': _hip.build_id(), 'has_kernel_path': has_kernel,
               'config': {'dim': D, 'hidden': [H], 'layers': a.layers, 'time_net': 'TimeTanh', 'rows': N, 'reps': a.reps, 'runs': a.runs}}
    for name, r in raw.items():
        out = {}
        for path, ts in r.items():
            if ts:
                out[path + '_ms'] = statistics.median(ts)
                out[path + '_spread_ms'] = max(ts) - min(ts)
                out[path + '_runs_ms'] = ts
        if has_kernel:
            out['composed_over_kernel'] = out['composed_ms'] / out['kernel_ms']
        results[name] = out
        print(name, json.dumps(out))
    # (c) one layer's backward alone, every gradient wanted
    params = [p for p in f.parameters()]

    def backward_only(module):
        module.zero_grad(set_to_none=True)
        y = module(x, t)
        return [timed(lambda: torch.autograd.grad(y, [x] + params, cot, retain_graph=True), a.reps) for _ in range(a.runs)]
    with Composed(f):
        comp = backward_only(f)
    out = {'composed_ms': statistics.median(comp), 'composed_spread_ms': max(comp) - min(comp)}
    if has_kernel:
        ker = backward_only(f)
        assert f._last_path == 'kernel'
        m = f.mask_vector(D)
        K, n_live = int((m > 0.5).sum()), int((m <= 0.5).sum())
        flop = N * 6 * (K * H + 2 * n_live * H)
        nbytes = N * 4 * (3 * D + 3)
        ms = statistics.median(ker)
        out.update({'kernel_ms': ms, 'kernel_spread_ms': max(ker) - min(ker), 'composed_over_kernel': out['composed_ms'] / ms, 'flop': flop,
                    'bytes': nbytes, 'tflops': flop / ms / 1e9, 'frac_of_fp32_mfma_peak': flop / (ms * 1e-3) / PEAK_F32_MFMA,
                    'tbytes_per_s': nbytes / ms / 1e9, 'frac_of_hbm_peak': nbytes / (ms * 1e-3) / PEAK_HBM})
    results['c_layer_backward_only'] = out
    print('c_layer_backward_only', json.dumps(out))
    if a.merge_parent:
        with open(a.merge_parent) as fh:
            parent = json.load(fh)
        assert parent['config'] == results['config'], 'the parent run used another configuration'
        results['parent_commit'] = {'build_id': parent['build_id'], **{name: parent[name] for name in list(cases) + ['c_layer_backward_only']}}
        print('parent_commit', json.dumps(results['parent_commit']))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
