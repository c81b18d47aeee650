"""Writes tests/golden/f23_cfg2_parent_bits.npz: the outputs of the library this script is run against on fixture F4's flow
(tests/golden/f4_cfg2.npz), with fp32 and with bf16 x storage -- outputs only.  tests/test_gpu_cfg2_kstep.py holds later builds to
these bits: run it against the PARENT of a change that re-schedules the cfg 2 step without changing its arithmetic
(STRIBOR_HIP_LIB=<parent library> python tools/make_parent_bits.py [out.npz])."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import stribor_amd as st  # noqa: E402
from goldens import Golden  # noqa: E402
from producthelp import product_flow  # noqa: E402
from stribor_amd import _hip  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'f23_cfg2_parent_bits.npz')
    g = Golden('f4_cfg2')
    st.set_gemm_precision('fast')
    arrays = {}
    with torch.no_grad():
        flow = product_flow(g, 'cfg2')
        x = g.t('cfg2/x').cuda()
        for tag, xin in (('f32', x), ('bf16', x.bfloat16())):
            arrays[tag + '/log_prob'] = flow.log_prob(xin).float().cpu().numpy()
            arrays[tag + '/forward'] = flow.forward(xin)[:257].float().cpu().numpy()
            arrays[tag + '/inverse'] = flow.inverse(xin)[:257].float().cpu().numpy()
    meta = {'source': 'f4_cfg2', 'case': 'cfg2', 'precision': 'fast', 'build_id': _hip.build_id(),
            'note': 'bf16/*: x stored bf16; bf16 outputs widened to fp32 (exact)'}
    np.savez_compressed(out, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print('wrote', out, {k: v.shape for k, v in arrays.items()}, meta['build_id'])


if __name__ == '__main__':
    main()
