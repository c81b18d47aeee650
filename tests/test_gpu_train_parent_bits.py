"""GPU: the three one-launch training backward kernels keep the bits of the build before their weight-gradient contraction moved into
stribor_amd/csrc/sx_train_contract.h (tests/golden/f25_train_parent_bits.npz, written by tools/make_train_parent_bits.py against the
parent's library).  The move changes no arithmetic -- every output element of the ordered sum is still one thread's fp64 sum over the
slots in slot order --, so every stored value must come out bit for bit (NaNs matching NaNs).  Cases: tests/trainbitshelp.py."""
import json
import os

import numpy as np
import pytest
import torch

import trainbitshelp as tb
from goldens import GOLDEN_DIR

pytestmark = pytest.mark.gpu

_golden = {}


def golden():
    if not _golden:
        z = np.load(os.path.join(GOLDEN_DIR, 'f25_train_parent_bits.npz'))
        _golden['meta'] = json.loads(bytes(z['meta']).decode())
        _golden['arrays'] = {k: torch.from_numpy(z[k]) for k in z.files if k != 'meta'}
    return _golden['meta'], _golden['arrays']


def _hold(case):
    _, want = golden()
    got = tb.run(case)
    stored = sorted(k[len(case) + 1:] for k in want if k.startswith(case + '/'))
    assert stored and sorted(got) == stored, (case, sorted(got), stored)
    bad = []
    for name in stored:
        a, b = got[name], want[f'{case}/{name}']
        differ = int(((a != b) & ~(a.isnan() & b.isnan())).sum()) if a.shape == b.shape else -1
        print(f'{case}/{name}: {differ} of {b.numel()} values differ from the parent build')
        if not tb.same_bits(a, b):
            bad.append((name, differ))
    assert not bad, (case, bad)


def test_the_fixture_holds_every_case():
    meta, want = golden()
    assert meta['cases'] == list(tb.CASES) and meta['multi'] == list(tb.MULTI)
    for case in meta['cases'] + meta['multi']:
        assert any(k.startswith(case + '/param') for k in want), case


@pytest.mark.parametrize('case', list(tb.CASES))
def test_one_pass_cases_keep_the_parents_bits(case):
    _hold(case)


@pytest.mark.parametrize('case', list(tb.MULTI))
def test_multi_pass_parameter_gradients_keep_the_parents_bits(case):
    meta, _ = golden()
    assert tb.cu_count() == meta['cu_count'], (
        f"this device has {tb.cu_count()} CUs, the fixture was written on {meta['cu_count']}: the multi-pass grids differ -- "
        'regenerate tests/golden/f25_train_parent_bits.npz with tools/make_train_parent_bits.py against the parent library')
    _hold(case)
