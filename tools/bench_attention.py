"""Timing of the attention core (sx_attention_fwd / sx_attention_bwd) and of net.SelfAttention, against the reference formula
(stribor/net/attention.py:26-49) composed in torch on the device, at (B, N, E, H) = (4096, 64, 64, 4), (256, 512, 64, 4) and
(16, 4096, 64, 4); and a 4-layer set flow (Coupling(Affine(latent_net=SelfAttention), set_data=True)) log_prob and training step
at B = 4096, N = 64, D = 8.  Device events around `--reps` calls after warm-up.

Algorithmic traffic of the core: q, k, v read and y written once (4 B H N dh per set each) plus the log-sum-exp; its backward
reads q, k, v, y, dy, lse and writes dq, dk, dv.  FLOPs: 4 B H N^2 dh forward (QK^T, PV) and 10 B H N^2 dh backward as executed
by the two passes (S and dP in each, dV, dK, dQ): 14 B H N^2 dh for forward + backward.
The bound is the larger of bytes / 5.3 TB/s and FLOPs / 157.3 TF (fp32 MFMA peak).

    python tools/bench_attention.py [--reps 20] [--json out.json] [--no-composition-large]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import stribor_amd as st
from stribor_amd.net.attention import _attention_composed
from stribor_amd.util import flowdesc as fd

PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 5.3e12
SHAPES = [(4096, 64, 64, 4), (256, 512, 64, 4), (16, 4096, 64, 4)]


def timed(fn, reps, warm=3):
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


def bound(nbytes, flops):
    tb, tf = nbytes / PEAK_HBM * 1e3, flops / PEAK_F32_MFMA * 1e3
    return {'bytes': nbytes, 'flops': flops, 'hbm_floor_ms': tb, 'mfma_floor_ms': tf, 'bound': 'hbm' if tb > tf else 'mfma'}


def fwd_bwd(fn, q, k, v, gy):
    def run():
        for t in (q, k, v):
            t.grad = None
        fn(q, k, v).backward(gy)
    return run


def core_shape(B, N, E, H, reps, composition):
    dh = E // H
    q, k, v = (torch.randn(B, N, E, device='cuda', requires_grad=True) for _ in range(3))
    gy = torch.randn(B, N, E, device='cuda')
    core = lambda a, b, c: st.net.attention(a, b, c, n_heads=H)
    comp = lambda a, b, c: _attention_composed(a, b, c, H, False, None)
    r = {'shape': [B, N, E, H]}
    with torch.no_grad():
        r['core_fwd_ms'] = timed(lambda: core(q, k, v), reps)
    r['core_fwd_bwd_ms'] = timed(fwd_bwd(core, q, k, v, gy), reps)
    io = 4 * B * N * E
    r['fwd'] = bound(4 * io + 4 * B * H * N, 4 * B * H * N * N * dh)
    r['fwd_bwd'] = bound(4 * io + 4 * B * H * N + (6 * io + 4 * B * H * N + 3 * io), 14 * B * H * N * N * dh)
    if composition:
        with torch.no_grad():
            r['composition_fwd_ms'] = timed(lambda: comp(q, k, v), max(2, reps // 4), warm=1)
        r['composition_fwd_bwd_ms'] = timed(fwd_bwd(comp, q, k, v, gy), max(2, reps // 4), warm=1)
        r['fwd_speedup'] = r['composition_fwd_ms'] / r['core_fwd_ms']
        r['fwd_bwd_speedup'] = r['composition_fwd_bwd_ms'] / r['core_fwd_bwd_ms']
    # the whole SelfAttention (one packed QKV GEMM, the core, proj) with the composition in place of the core
    torch.manual_seed(0)
    m = st.net.SelfAttention(E, [E], E, n_heads=H).to('cuda')
    x = torch.randn(B, N, E, device='cuda')
    with torch.no_grad():
        r['self_attention_fwd_ms'] = timed(lambda: m(x), reps)
    r['self_attention_fwd_bwd_ms'] = timed(lambda: m(x).sum().backward(), reps)
    if composition:
        def comp_model():
            return m.proj(_attention_composed(m.query(x), m.key(x), m.value(x), H, False, None))
        with torch.no_grad():
            r['self_attention_composition_fwd_ms'] = timed(comp_model, max(2, reps // 4), warm=1)
        r['self_attention_composition_fwd_bwd_ms'] = timed(lambda: comp_model().sum().backward(), max(2, reps // 4), warm=1)
    return r


def set_flow(reps):
    B, N, D = 4096, 64, 8
    masks = ['ordered_left_half', 'ordered_right_half', 'parity_even', 'parity_odd']
    desc = [{'kind': 'coupling_affine', 'dim': D, 'hidden': [64], 'mask': m, 'latent_dim': 0, 'set_data': True,
             'net': 'self_attention', 'n_heads': 4} for m in masks]
    torch.manual_seed(0)
    flow = fd.build_flow(st, desc, D).to('cuda')
    x = torch.randn(B, N, D, device='cuda')
    opt = torch.optim.Adam(flow.parameters(), lr=1e-4)

    def train_step():
        opt.zero_grad(set_to_none=True)
        loss = -flow.log_prob(x).mean()
        loss.backward()
        opt.step()
    with torch.no_grad():
        lp = timed(lambda: flow.log_prob(x), reps)
    tr = timed(train_step, reps)
    return {'B': B, 'N': N, 'D': D, 'layers': 4, 'conditioner': 'SelfAttention(8, [64], 16, n_heads=4)', 'log_prob_ms': lp,
            'train_step_ms': tr}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    ap.add_argument('--no-composition-large', action='store_true', help='skip the composition at N = 4096 (17 GB of scores)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_attention needs a GPU'
    out = {'shapes': []}
    for B, N, E, H in SHAPES:
        comp = not (a.no_composition_large and N >= 4096)
        r = core_shape(B, N, E, H, a.reps if N < 4096 else max(3, a.reps // 4), comp)
        out['shapes'].append(r)
        line = (f'B={B} N={N} E={E} H={H}: core fwd {r["core_fwd_ms"]:.3f} ms (floor {max(r["fwd"]["hbm_floor_ms"], r["fwd"]["mfma_floor_ms"]):.3f}, '
                f'{r["fwd"]["bound"]}), fwd+bwd {r["core_fwd_bwd_ms"]:.3f} ms; SelfAttention fwd {r["self_attention_fwd_ms"]:.3f} ms, '
                f'fwd+bwd {r["self_attention_fwd_bwd_ms"]:.3f} ms')
        if comp:
            line += (f'; composition fwd {r["composition_fwd_ms"]:.3f} ms ({r["fwd_speedup"]:.2f} x), fwd+bwd '
                     f'{r["composition_fwd_bwd_ms"]:.3f} ms ({r["fwd_bwd_speedup"]:.2f} x)')
        print(line, flush=True)
        torch.cuda.empty_cache()
    out['set_flow'] = set_flow(a.reps)
    print(f'set flow 4 x SelfAttention coupling, B=4096 N=64 D=8: log_prob {out["set_flow"]["log_prob_ms"]:.3f} ms, '
          f'training step {out["set_flow"]["train_step_ms"]:.3f} ms', flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
