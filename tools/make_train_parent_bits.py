"""Writes tests/golden/f25_train_parent_bits.npz: what the library this script is run against produces on the cases of
tests/trainbitshelp.py -- the three one-launch training backward kernels at the smallest shapes that reach each piece of their shared
weight-gradient contraction, and one multi-pass batch each.  tests/test_gpu_train_parent_bits.py holds later builds to these bits: run
it against the PARENT of a change that moves that code without changing its arithmetic
(STRIBOR_HIP_LIB=<parent library> python tools/make_train_parent_bits.py [out.npz]).  The multi-pass cases' grids depend on the
device's CU count, which the meta records: regenerate on a device that differs."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import trainbitshelp as tb  # noqa: E402
from stribor_amd import _hip  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'f25_train_parent_bits.npz')
    arrays = {}
    for case in list(tb.CASES) + list(tb.MULTI):
        for name, t in tb.run(case).items():
            arrays[f'{case}/{name}'] = t.numpy()
    meta = {'build_id': _hip.build_id(), 'library': os.path.basename(_hip.LIB_PATH), 'cu_count': tb.cu_count(),
            'cases': list(tb.CASES), 'multi': list(tb.MULTI)}
    np.savez_compressed(out, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print('wrote', out, len(arrays), 'arrays', sum(a.nbytes for a in arrays.values()), 'bytes raw', meta['build_id'], 'CUs', meta['cu_count'])


if __name__ == '__main__':
    main()
