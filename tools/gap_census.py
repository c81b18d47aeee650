#!/usr/bin/env python3
"""Where a coupling step's vector work stands relative to its MFMAs, read from a kernel's assembly (hipcc -S).

On gfx950 a wave's vector instructions overlap the matrix pipe only in the shadow of that wave's OWN MFMAs (DESIGN 4.1,
tools/coexec_probe.hip): about 24 issue cycles per 32-cycle MFMA, a transcendental costing 8 and any other vector instruction 4.
Per coupling arm -- a basic block that holds MFMAs -- this prints

  * the issue cycles of vector work between consecutive MFMAs (the gap list), in front of the first and behind the last,
  * how many gaps are empty (bare) and how many hold more than the shadow (over-full),
  * the cycles hidden when every gap is capped at the shadow,
  * the multiset of v_* mnemonics and the number of ds_read instructions of the body.

Only v_* and ds_read mnemonics are looked at.  The assembly of the headline kernel:

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -mllvm -amdgpu-atomic-optimizer-strategy=None -DSX_F16X3 \\
        -DSX_FAMILY=0 -DSX_TX=2 -DSX_HT=2 -DSX_ONLY_MODE=5 --offload-device-only -S sx_flow_inst.hip -o m5.s
  python tools/gap_census.py m5.s [--json] [--min-mfma 36] [--compare other.s]

--compare: exit status 1 unless both files hold the same arms (count, MFMAs per arm) and no path through an arm holds MORE of any v_*
mnemonic than in OTHER.  A path is the whole file less the other arms: a rider that one build keeps inside each arm -- the log-det
adds -- another build leaves once to the step loop's tail, so arms alone do not compare.  Every difference is listed; v_mov_* is
register traffic and is listed but not judged.
"""
import argparse
import collections
import json
import re
import sys

SHADOW = 24
TRANS = ('v_exp_', 'v_rcp_', 'v_log_', 'v_sqrt_', 'v_rsq_', 'v_sin_', 'v_cos_')
_LABEL = re.compile(r'^(\.LBB\d+_\d+:|; %bb\.\d+:|[A-Za-z_][\w$.]*:)')
_INSN = re.compile(r'^\s+([a-z_][a-z0-9_]*)\b')
_BRANCH = ('s_cbranch', 's_branch', 's_endpgm', 's_setpc', 's_swappc')


def cost(mnemonic):
    return 8 if mnemonic.startswith(TRANS) else 4


def blocks(lines):
    """Basic blocks as lists of mnemonics: a label opens one, a branch closes one."""
    cur = []
    for ln in lines:
        if _LABEL.match(ln):
            if cur:
                yield cur
            cur = []
            continue
        m = _INSN.match(ln)
        if not m or ln.lstrip().startswith(('.', ';')):
            continue
        cur.append(m.group(1))
        if m.group(1).startswith(_BRANCH):
            yield cur
            cur = []
    if cur:
        yield cur


def census(block):
    gaps, acc, n_mfma, pre = [], 0, 0, 0
    mix, reads = collections.Counter(), 0
    for op in block:
        if op.startswith('v_mfma'):
            if n_mfma == 0:
                pre = acc
            else:
                gaps.append(acc)
            acc, n_mfma = 0, n_mfma + 1
            mix[op] += 1
        elif op.startswith('v_'):
            acc += cost(op)
            mix[op] += 1
        elif op.startswith('ds_read'):
            reads += 1
    return {'mfma': n_mfma, 'pre': pre, 'gaps': gaps, 'post': acc,
            'bare': sum(g == 0 for g in gaps), 'bare_at': [i for i, g in enumerate(gaps) if g == 0],
            'over_full': sum(g > SHADOW for g in gaps),
            'hidden': sum(min(g, SHADOW) for g in gaps), 'available': SHADOW * len(gaps),
            'valu_cycles': pre + sum(gaps) + acc, 'ds_read': reads, 'v_mix': dict(sorted(mix.items()))}


def arms(path, min_mfma):
    with open(path) as f:
        return [c for c in (census(b) for b in blocks(f)) if c['mfma'] >= min_mfma]


def file_mix(path):
    mix = collections.Counter()
    with open(path) as f:
        for b in blocks(f):
            mix.update(op for op in b if op.startswith('v_'))
    return mix


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('asm')
    ap.add_argument('--min-mfma', type=int, default=36, help='a block with at least this many MFMAs is an arm')
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--compare', metavar='OTHER', help='require the same arms with equal v_* multisets as in OTHER')
    a = ap.parse_args()
    got = arms(a.asm, a.min_mfma)
    if a.json:
        print(json.dumps(got))
    else:
        for i, c in enumerate(got):
            print(f'arm {i}: {c["mfma"]} MFMAs, {c["ds_read"]} ds_read, vector issue {c["valu_cycles"]} cycles')
            print(f'  before first {c["pre"]}, behind last {c["post"]}')
            print('  gaps ' + ' '.join(str(g) for g in c['gaps']))
            print(f'  bare {c["bare"]} (at {c["bare_at"]}), over-full {c["over_full"]}, hidden at the {SHADOW}-cycle cap '
                  f'{c["hidden"]} of {c["available"]}')
            print('  ' + ' '.join(f'{k}:{v}' for k, v in c['v_mix'].items()))
    if a.compare:
        other = arms(a.compare, a.min_mfma)
        same = [c['mfma'] for c in got] == [c['mfma'] for c in other]
        if same:
            def paths(path, cs):
                total = file_mix(path)
                return [total - sum((collections.Counter(d['v_mix']) for j, d in enumerate(cs) if j != i), collections.Counter())
                        for i in range(len(cs))]
            for i, (mine, theirs) in enumerate(zip(paths(a.asm, got), paths(a.compare, other))):
                for k in sorted(set(mine) | set(theirs)):
                    if mine[k] != theirs[k]:
                        print(f'  path through arm {i}: {k} {mine[k]} vs {theirs[k]}')
                        same = same and (mine[k] < theirs[k] or k.startswith('v_mov_'))
        print(('no v_* work beyond ' if same else 'arms or v_* work DIFFER from ') + a.compare)
        if not same:
            sys.exit(1)


if __name__ == '__main__':
    main()
