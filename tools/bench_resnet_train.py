"""Timing of ContinuousIResNet TRAINING on sx_resnet_flow_bwd: dim 64, hidden [64, 64], TimeTanh, 2^18 rows, training mode, after a
warm-up of the power iteration.  Three cases, each forward + backward, device events around `REPS` steps:

    (a) f(x, t)                       (b) f.inverse(y, t) at 100 iterations            (c) a NeuralFlow of four such layers, one step
                                                                                          (forward, loss, backward, SGD update)

Each case runs on the kernel path and on the composition path of the same build (the planner `_train_plan` patched to None), in
`--runs` alternating runs of one warm-up step and `--reps` timed steps each, the same for both paths; the figures are the median
and the spread (max - min) over the runs.  On a build without the kernel path (no `_train_plan`) only the composition path is
timed: run the tool from a checkout of the parent commit with --json, then pass that file to this build's run as --merge-parent,
which copies its three cases into the result as `parent_commit`.

FLOP count of (b)'s backward: the implicit iteration makes `iterations` transpose products of three 64 x 64 layers per row, the
forward inverse's 2^18 x 100 x 24576 = 6.4e11 FLOP, 4.1 ms at the 157.3 TF fp32-MFMA peak; the backward alone is timed for that.

    python tools/bench_resnet_train.py [--rows 262144] [--iterations 100] [--json profiles/resnet_train_bench.json]
                                       [--merge-parent parent_run.json]
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

PEAK_F32_MFMA = 157.3e12


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
    """Inside: every IResNet layer under `module` takes the composition path."""

    def __init__(self, module):
        self.mods = [m for m in module.modules() if hasattr(m, '_train_plan')]

    def __enter__(self):
        for m in self.mods:
            m._train_plan = lambda: None

    def __exit__(self, *exc):
        for m in self.mods:
            del m._train_plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 18)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--hidden', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--merge-parent', default=None, help="a --json result of this tool run on the parent commit's checkout")
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_resnet_train needs a GPU'
    torch.manual_seed(0)
    D, H, N, K = a.dim, a.hidden, a.rows, a.iterations

    def layer():
        f = st.ContinuousIResNet(D, [H, H], time_net=st.net.TimeTanh(D)).to('cuda')
        with torch.no_grad():
            for _ in range(5):                   # settle the power iteration (sigma then bounds the Lipschitz constant)
                f(torch.randn(1024, D, device='cuda'), t=torch.rand(1024, 1, device='cuda'))
        return f.train()

    f = layer()
    nf = st.NeuralFlow([layer() for _ in range(4)]).to('cuda').train()
    opt = torch.optim.SGD(nf.parameters(), lr=0.0)
    has_kernel = hasattr(f, '_train_plan')
    x = torch.randn(N, D, device='cuda', requires_grad=True)
    t = torch.rand(N, 1, device='cuda')
    cot = torch.randn(N, D, device='cuda')

    def step_a():
        f.zero_grad(set_to_none=True)
        x.grad = None
        f(x, t=t).backward(cot)

    def step_b():
        f.zero_grad(set_to_none=True)
        x.grad = None
        f.inverse(x, t=t, iterations=K).backward(cot)

    def step_c():
        opt.zero_grad(set_to_none=True)
        x.grad = None
        nf(x, t=t).square().mean().backward()
        opt.step()

    cases = {'a_forward': (step_a, f), 'b_inverse': (step_b, f), 'c_neural_flow4': (step_c, nf)}
    raw = {name: {'kernel': [], 'composed': []} for name in cases}
    for _ in range(a.runs):                      # alternating runs: kernel, composed, kernel, ...
        for name, (step, module) in cases.items():
            if has_kernel:
                raw[name]['kernel'].append(timed(step, a.reps))
                assert all(m._last_grad_path == 'kernel' for m in module.modules() if hasattr(m, '_last_grad_path'))
            with Composed(module):
                raw[name]['composed'].append(timed(step, a.reps))
    results = {'build_id': _hip.build_id(), 'has_kernel_path': has_kernel,
               'config': {'dim': D, 'hidden': [H, H], 'time_net': 'TimeTanh', 'rows': N, 'iterations': K, 'mode': 'train', 'reps': a.reps,
                          'runs': a.runs}}
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
    if has_kernel:
        # (b)'s backward alone: the sigma row, ONE sx_resnet_flow_bwd call (its kernel and the ordered sum) and the few D x D host ops
        f.zero_grad(set_to_none=True)
        xo = f.inverse(x, t=t, iterations=K)
        params = [p for p in f.parameters()]
        bwd = [timed(lambda: torch.autograd.grad(xo, [x] + params, cot, retain_graph=True), a.reps) for _ in range(a.runs)]
        flop = N * K * 2 * (D * H + H * H + H * D)
        ms = statistics.median(bwd)
        results['b_inverse_backward_only'] = {'ms': ms, 'spread_ms': max(bwd) - min(bwd), 'flop': flop, 'tflops': flop / ms / 1e9,
                                              'frac_of_fp32_mfma_peak': flop / (ms * 1e-3) / PEAK_F32_MFMA}
        print('b_inverse_backward_only', json.dumps(results['b_inverse_backward_only']))
    if a.merge_parent:
        with open(a.merge_parent) as fh:
            parent = json.load(fh)
        assert parent['config'] == results['config'], 'the parent run used another configuration'
        results['parent_commit'] = {'build_id': parent['build_id'], **{name: parent[name] for name in cases}}
        print('parent_commit', json.dumps(results['parent_commit']))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
