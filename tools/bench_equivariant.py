"""Timing of net.EquivariantNet (Deep Sets) on sx_equivariant_fwd / sx_equivariant_bwd against the torch op sequence it replaces.

    (a) EquivariantNet(8 + 2, [64, 64], 16) on (B, N) = (4096, 64): forward (no grad), and forward + backward (x and every parameter)
    (b) 4 x Coupling(Affine(8, latent_net=EquivariantNet(8, [64], 16)), 'ordered_left_half', set_data=True) under a unit normal at
        B = 4096, N = 64: log_prob (no grad) and one Adam step -- the README set-flow line's shape with the other conditioner
    (c) EquivariantNet(8, [32, 32], 16) on the same rows: a shape inside the backward kernel's coverage with two hidden layers

Each case runs on `forward` (the kernel where the planner covers the call; `path` records what ran) and on the baseline: the parent
commit's module, whose op sequence survives verbatim as `forward_twice_differentiable` -- `forward` is patched to it for the
baseline runs, so both are timed in the same process, in `--runs` alternating runs of one warm-up call and `--reps` timed calls
each, device events around the timed calls; the figures are the median and the spread (max - min) over the runs.  On a build
without the kernel (no `kernel_plan`) only the module itself is timed: run the tool from a checkout of the parent commit with
--json, then pass that file to this build's run as --merge-parent, which copies its cases into the result as `parent_commit`.

    python tools/bench_equivariant.py [--sets 4096] [--set-size 64] [--json profiles/equivariant_bench.json] [--merge-parent parent_run.json]
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
from stribor_amd.net.equivariant import EquivariantNet


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


class Baseline:
    """Inside: every EquivariantNet runs the torch op sequence (the parent commit's forward)."""

    def __enter__(self):
        self.forward = EquivariantNet.forward
        EquivariantNet.forward = EquivariantNet.forward_twice_differentiable

    def __exit__(self, *exc):
        EquivariantNet.forward = self.forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sets', type=int, default=4096)
    ap.add_argument('--set-size', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--merge-parent', default=None, help="a --json result of this tool run on the parent commit's checkout")
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_equivariant needs a GPU'
    torch.manual_seed(0)
    B, N = a.sets, a.set_size
    has_kernel = hasattr(EquivariantNet, 'kernel_plan')

    net_a = EquivariantNet(8 + 2, [64, 64], 16).to('cuda')
    net_c = EquivariantNet(8, [32, 32], 16).to('cuda')
    flow = st.NormalizingFlow(st.UnitNormal(8), [st.Coupling(st.Affine(8, latent_net=EquivariantNet(8, [64], 16)), 'ordered_left_half', set_data=True)
                                      for _ in range(4)]).to('cuda')
    opt = torch.optim.Adam(flow.parameters(), lr=1e-4)
    xa = torch.randn(B, N, 10, device='cuda')
    xc = torch.randn(B, N, 8, device='cuda')
    ga, gc = torch.randn(B, N, 16, device='cuda'), torch.randn(B, N, 16, device='cuda')

    def fwd(net, x):
        def run():
            with torch.no_grad():
                net(x)
        return run

    def fwd_bwd(net, x, g):
        xg = x.clone().requires_grad_(True)

        def run():
            net.zero_grad(set_to_none=True)
            xg.grad = None
            net(xg).backward(g)
        return run

    def log_prob():
        with torch.no_grad():
            flow.log_prob(xc)

    def adam_step():
        opt.zero_grad(set_to_none=True)
        (-flow.log_prob(xc).mean()).backward()
        opt.step()

    nets_b = [m for m in flow.modules() if isinstance(m, EquivariantNet)]
    cases = {'a_forward': (fwd(net_a, xa), [net_a]), 'a_forward_backward': (fwd_bwd(net_a, xa, ga), [net_a]),
             'b_log_prob': (log_prob, nets_b), 'b_adam_step': (adam_step, nets_b),
             'c_forward': (fwd(net_c, xc), [net_c]), 'c_forward_backward': (fwd_bwd(net_c, xc, gc), [net_c])}
    raw = {name: {'forward': [], 'torch_sequence': []} for name in cases}
    paths = {}
    for _ in range(a.runs):                      # alternating runs: forward, the torch sequence, forward, ...
        for name, (step, nets) in cases.items():
            raw[name]['forward'].append(timed(step, a.reps))
            paths[name] = sorted({getattr(n, '_last_path', None) or 'composed' for n in nets})
            if has_kernel:
                with Baseline():
                    raw[name]['torch_sequence'].append(timed(step, a.reps))
    results = {'build_id': _hip.build_id(), 'has_kernel_path': has_kernel,
               'config': {'sets': B, 'set_size': N, 'reps': a.reps, 'runs': a.runs,
                          'a': 'EquivariantNet(10, [64, 64], 16)', 'b': '4 x Coupling(Affine(8, EquivariantNet(8, [64], 16)), set_data=True)',
                          'c': 'EquivariantNet(8, [32, 32], 16)'}}
    for name, r in raw.items():
        out = {'path': paths[name]}
        for which, ts in r.items():
            if ts:
                out[which + '_ms'] = statistics.median(ts)
                out[which + '_spread_ms'] = max(ts) - min(ts)
                out[which + '_runs_ms'] = ts
        if has_kernel:
            out['torch_sequence_over_forward'] = out['torch_sequence_ms'] / out['forward_ms']
        results[name] = out
        print(name, json.dumps(out))
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
