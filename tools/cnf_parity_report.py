"""Worst err / bound of sx_cnf_flow over the F16 fixture cases, for profiles/cnf_parity_ratios.txt.

Per case and quantity (y, log-det, forward and reverse): err = max |kernel - fp64|, bound = max(8 x max |fixture - fp64|,
1e-6 x max(1, max |fp64|)) -- the rule of tests/test_gpu_cnf.py, from the same helpers.

    python tools/cnf_parity_report.py [--out profiles/cnf_parity_ratios.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import torch

import cnfhelp as ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    g, rows = ch.golden(), []
    for case in ch.case_names():
        f, x, lat, _ = ch.build_case(case)
        yb = g.t(f'{case}/y')
        truth = ch.solve64(f, x, lat) + ch.solve64(f, yb, lat, reverse=True)
        f = f.to('cuda')
        kw = {} if lat is None else {'latent': lat.to('cuda')}
        with torch.no_grad():
            got = f.forward_and_log_det_jacobian(x.to('cuda'), **kw) + f.inverse_and_log_det_jacobian(yb.to('cuda'), **kw)
        assert f._last_path == 'kernel'
        for name, a_, t in zip(('y', 'ldj', 'x_back', 'ldj_back'), got, truth):
            tol, e_ref = ch.bound(g.t(f'{case}/{name}'), t)
            err = (a_.cpu().double() - t).abs().max().item()
            rows.append((err / tol, err / e_ref if e_ref else float('inf'), case, name, err, e_ref, tol))
    rows.sort(reverse=True)
    lines = [f'sx_cnf_flow against fixture F16: {len(rows)} (case, quantity) pairs, worst err / bound = {rows[0][0]:.3f}',
             'err / bound   err / e_ref   case  quantity  err  e_ref  bound']
    lines += [f'{r[0]:.3f}  {r[1]:.2f}  {r[2]}  {r[3]}  {r[4]:.3e}  {r[5]:.3e}  {r[6]:.3e}' for r in rows[:12]]
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
