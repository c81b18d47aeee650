"""Writes tests/golden/f26_spline_parent_bits.npz: what the library this script is run against produces on the cases of
tests/splinebitshelp.py -- every kernel that reads the spline arithmetic of sx_rqs_core.h / sx_cubic_core.h and the transcendental
helpers of sx_common.h.  tests/test_gpu_spline_parent_bits.py holds later builds to these bits: run it against the PARENT of a change
that moves that code without changing its arithmetic
(STRIBOR_HIP_LIB=<parent library> python tools/make_spline_parent_bits.py [out.npz]).  Every case runs twice; an array the library
itself does not reproduce bit for bit is left out and named in the meta under `unstable` -- allowed only for the slab backward's
parameter gradients (float atomics), anything else is an error."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import splinebitshelp as sb  # noqa: E402
from stribor_amd import _hip  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'f26_spline_parent_bits.npz')
    arrays, unstable = {}, []
    for case in sb.CASES:
        first, second = sb.run(case), sb.run(case)
        assert sorted(first) == sorted(second), case
        for name, t in first.items():
            if sb.same_bits(t, second[name]):
                arrays[f'{case}/{name}'] = t.numpy()
            else:
                assert sb.may_be_unstable(case, name), f'{case}/{name}: two runs of this library differ'
                unstable.append(f'{case}/{name}')
    meta = {'build_id': _hip.build_id(), 'library': os.path.basename(_hip.LIB_PATH), 'cu_count': sb.cu_count(),
            'cases': list(sb.CASES), 'cu_cases': list(sb.CU_CASES), 'unstable': unstable}
    np.savez_compressed(out, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print('wrote', out, len(arrays), 'arrays', sum(a.nbytes for a in arrays.values()), 'bytes raw', meta['build_id'], 'CUs', meta['cu_count'],
          'unstable', unstable)


if __name__ == '__main__':
    main()
