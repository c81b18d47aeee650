"""GPU: the spline kernels keep the bits of the build before their copied constants, closing form, bin sweeps and transcendental
helpers moved into stribor_amd/csrc/sx_rqs_core.h, sx_cubic_core.h and sx_common.h (tests/golden/f26_spline_parent_bits.npz, written
by tools/make_spline_parent_bits.py against the parent's library).  The move changes no arithmetic, so every stored value must come
out bit for bit (NaNs matching NaNs).  Cases: tests/splinebitshelp.py."""
import json
import os

import numpy as np
import pytest
import torch

import splinebitshelp as sb
from goldens import GOLDEN_DIR

pytestmark = pytest.mark.gpu

_golden = {}


def golden():
    if not _golden:
        z = np.load(os.path.join(GOLDEN_DIR, 'f26_spline_parent_bits.npz'))
        _golden['meta'] = json.loads(bytes(z['meta']).decode())
        _golden['arrays'] = {k: torch.from_numpy(z[k]) for k in z.files if k != 'meta'}
    return _golden['meta'], _golden['arrays']


def test_the_fixture_holds_every_case():
    meta, want = golden()
    assert meta['cases'] == list(sb.CASES) and meta['cu_cases'] == list(sb.CU_CASES)
    for case in meta['cases']:
        assert any(k.startswith(case + '/') for k in want), case
    for name in meta['unstable']:                     # only parameter gradients of the slab backward may be missing
        case, _, array = name.rpartition('/')
        assert sb.may_be_unstable(case, array) and name not in want, name


@pytest.mark.parametrize('case', list(sb.CASES))
def test_cases_keep_the_parents_bits(case):
    meta, want = golden()
    if case in sb.CU_CASES:
        assert sb.cu_count() == meta['cu_count'], (
            f"this device has {sb.cu_count()} CUs, the fixture was written on {meta['cu_count']}: this case's grid differs -- "
            'regenerate tests/golden/f26_spline_parent_bits.npz with tools/make_spline_parent_bits.py against the parent library')
    got = sb.run(case)
    stored = sorted(k[len(case) + 1:] for k in want if k.startswith(case + '/'))
    left_out = sorted(k[len(case) + 1:] for k in meta['unstable'] if k.startswith(case + '/'))
    assert stored and sorted(got) == sorted(stored + left_out), (case, sorted(got), stored, left_out)
    bad = []
    for name in stored:
        a, b = got[name], want[f'{case}/{name}']
        differ = int(((a != b) & ~(a.isnan() & b.isnan())).sum()) if a.shape == b.shape else -1
        print(f'{case}/{name}: {differ} of {b.numel()} values differ from the parent build')
        if not sb.same_bits(a, b):
            bad.append((name, differ))
    assert not bad, (case, bad)
