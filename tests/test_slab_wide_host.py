"""CPU: the host side of the slab forward tier's wide form (rational-quadratic couplings of 17 .. 32 bins behind conditioners of up to
256 hidden units): the exports, the slot map, the validator of sx_rqs_slab_wide_fwd through ctypes (no call reaches a launch), the
planner's gate, and the host code under sanitizers (a stand-alone program)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.flows.spline import slab_slot_rows, slab_slot_rows_wide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sx_rqs_slab_wide_slots', 'sx_rqs_slab_wide_fwd_scratch_floats', 'sx_rqs_slab_wide_fwd')
CPU = torch.device('cpu')


def test_entry_points_declared_listed_exported_and_built():
    hdr = open(os.path.join(ROOT, 'include', 'stribor_hip.h')).read()
    declared = set(re.findall(r'\b(sx_[a-z0-9_]+)\s*\(', hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert 'asan_slab_wide' in open(os.path.join(ROOT, 'stribor_amd', 'csrc', 'Makefile')).read()
    assert _hip.lib().sx_abi_version() == 3 and re.search(r'#define SX_ABI_VERSION\s+3\b', hdr)


def test_size_queries():
    lib = _hip.lib()
    for n_live in (1, 2, 33, 1 << 20):
        assert lib.sx_rqs_slab_wide_slots(n_live) == n_live * 96
        assert lib.sx_rqs_slab_wide_fwd_scratch_floats(2049, n_live) == n_live * 2049
    assert lib.sx_rqs_slab_wide_slots(0) == 0 and lib.sx_rqs_slab_wide_slots(-5) == 0 and lib.sx_rqs_slab_wide_slots((1 << 20) + 1) == 0
    assert lib.sx_rqs_slab_wide_fwd_scratch_floats(-1, 4) == 0 and lib.sx_rqs_slab_wide_fwd_scratch_floats(1 << 36, 4) == 0
    assert lib.sx_rqs_slab_wide_fwd_scratch_floats(100, 0) == 0
    # the narrow form's queries answer as before
    assert lib.sx_rqs_slab_slots(33) == 17 * 96 and lib.sx_rqs_slab_fwd_scratch_floats(2049, 33) == 17 * 2049


@pytest.mark.parametrize('K', [17, 24, 31, 32])
@pytest.mark.parametrize('n_live', [1, 2, 33])
def test_slot_map_of_the_wide_form(n_live, K):
    """Slot 32 t + R of slab s holds parameter 16 ((R>>2)&1) + (R&3) + 4 (R>>3) of tile t (widths | heights | derivatives) of column s:
    every row ci (3K-1) + ... of the compact parameter block exactly once, -1 in the pads."""
    rows = slab_slot_rows_wide(n_live, K)
    assert rows.shape == (n_live * 96,) and rows.dtype == np.int32
    assert rows.shape[0] == _hip.lib().sx_rqs_slab_wide_slots(n_live)
    P = 3 * K - 1
    used = rows[rows >= 0]
    assert sorted(used.tolist()) == list(range(n_live * P))                   # every row, once
    for s in range(n_live):
        for t in range(3):
            for R in range(32):
                k = 16 * ((R >> 2) & 1) + (R & 3) + 4 * (R >> 3)
                want = s * P + t * K + k if k < (K - 1 if t == 2 else K) else -1
                assert rows[s * 96 + 32 * t + R] == want, (s, t, R)
    # in MFMA C-fragment order (register r of lane half hh = tile row 8 (r>>2) + 4 hh + (r&3)) half hh holds bins 16 hh .. 16 hh + 15
    for hh in range(2):
        for r in range(16):
            R = 8 * (r >> 2) + 4 * hh + (r & 3)
            k = 16 * hh + r
            assert rows[R] == (k if k < K else -1) and rows[32 + R] == (K + k if k < K else -1)
            assert rows[64 + R] == (2 * K + k if k < K - 1 else -1)


def test_narrow_slot_map_is_unchanged():
    rows = slab_slot_rows(3, 16)
    assert rows.shape == (2 * 96,) and sorted(rows[rows >= 0].tolist()) == list(range(3 * 47))
    assert rows[4] == 47 and rows[32 + 4] == 47 + 16                          # slot R = 4: parameter 0 of column 1


def _call(**over):
    """sx_rqs_slab_wide_fwd with valid arguments (host memory stands in for device memory: refused calls and n_rows = 0 return before
    any launch), one of them replaced."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    a = dict(x=p, h=p, ld_h=64, hidden=64, w_fwd=p, y=p, ldj=None, live_idx=None, live_start=32, n_live=32, pass_idx=None, n_pass=0,
             n_bins=24, left=-3.0, right=3.0, bottom=-3.0, top=3.0, n_rows=0, dim=64, reverse=1, ldj_scale=1.0, ldj_accumulate=0,
             h_fragments=0, scratch=None, err_flag=None, stream=None)
    for k, v in over.items():
        if v == 'buf':
            v = p
        assert k in a, k
        a[k] = v
    return _hip.lib().sx_rqs_slab_wide_fwd(*a.values()), buf


def test_validator_without_a_device():
    """tests/asan_driver.cpp:545-558 for the wide entry: every SX_REQUIRE of sx_rqs_slab_fwd applies, the bin range is 17 .. 32."""
    lib = _hip.lib()
    for K in (17, 24, 32):
        for rev in (0, 1):
            assert _call(n_bins=K, reverse=rev)[0] == 0                       # n_rows = 0: OK before any launch
    assert _call(ldj='buf', scratch='buf', pass_idx='buf', n_pass=32)[0] == 0
    assert _call(h_fragments=1, ld_h=0, hidden=256)[0] == 0
    bad = [dict(n_bins=16), dict(n_bins=33), dict(n_bins=0), dict(hidden=257, ld_h=320), dict(hidden=0), dict(ld_h=32),
           dict(n_live=65), dict(n_live=0), dict(left=3.0, right=-3.0), dict(bottom=3.0, top=3.0), dict(reverse=2), dict(reverse=-1),
           dict(ldj='buf'),                                                   # the row log-det needs the scratch buffer
           dict(pass_idx='buf', n_pass=33), dict(n_pass=5), dict(n_pass=-1), dict(n_rows=-1), dict(n_rows=1 << 36), dict(dim=0),
           dict(x=None), dict(h=None), dict(w_fwd=None), dict(y=None)]
    for over in bad:
        for n_rows in ((over['n_rows'],) if 'n_rows' in over else (0, 4)):    # refused before the n_rows = 0 return, and before a launch
            rc, _ = _call(**dict(over, n_rows=n_rows))
            assert rc != 0, over
            assert lib.sx_last_error(), over
    rc, buf = _call(n_bins=24)
    misaligned = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16 + 4
    assert _call(w_fwd=misaligned)[0] != 0
    assert _call(h=misaligned, h_fragments=1)[0] != 0
    # sx_rqs_slab_fwd keeps its contract: 17 bins are refused there
    assert lib.sx_rqs_slab_fwd(buf, buf, 64, 64, buf, buf, None, None, 32, 32, None, 0, 17, -3.0, 3.0, -3.0, 3.0, 0, 64, 1, 1.0, 0, 0, 0,
                               None, None, None) != 0


def _coupling(dim, hidden, K, spline_type='quadratic'):
    P = 3 * K - 1 if spline_type == 'quadratic' else 2 * K + 2
    net = st.net.MLP(dim, [hidden], dim * P)
    return st.Coupling(st.Spline(dim, K, latent_net=net, lower=-3, upper=3, spline_type=spline_type), mask='ordered_right_half')


def test_planner_gate_on_the_cpu_device():
    plan = _coupling(64, 160, 24)._spline_slab_plan(64, 0, CPU)
    progs, in_slots, slot_rows, hid_idx, live_idx, live_start, n_live, H, cache = plan
    assert (n_live, H, live_start) == (32, 160, 0) and cache.get('wide') is True and in_slots is not None and progs == []
    assert slot_rows.shape == (32 * 96,)
    # slot -> row of the last Linear: the transformed columns' rows (flows/spline.py:82-86), each once
    got = slot_rows[slot_rows >= 0].sort().values
    assert torch.equal(got, torch.arange(32 * 71, dtype=got.dtype))
    for K in (17, 32):
        assert _coupling(64, 256, K)._spline_slab_plan(64, 0, CPU)[-1].get('wide') is True
    narrow = _coupling(64, 160, 16)._spline_slab_plan(64, 0, CPU)
    assert 'wide' not in narrow[-1] and narrow[2].shape == (16 * 96,)
    with pytest.raises(NotImplementedError):
        _coupling(64, 160, 24, 'cubic')._spline_slab_plan(64, 0, CPU)
    with pytest.raises(NotImplementedError):
        _coupling(64, 257, 24)._spline_slab_plan(64, 0, CPU)
    with pytest.raises(NotImplementedError):
        _coupling(64, 160, 33)._spline_slab_plan(64, 0, CPU)


def test_validator_under_address_and_ub_sanitizers():
    """`make asan_slab_wide`: the library's host code (--offload-host-only, -fsanitize=address,undefined) linked with
    tests/asan_slab_wide_driver.cpp, a stand-alone program that drives the size functions and the validator without a GPU."""
    csrc = os.path.join(ROOT, 'stribor_amd', 'csrc')
    b = subprocess.run(['make', '-C', csrc, '-j', str(min(8, os.cpu_count() or 1)), 'asan_slab_wide'], capture_output=True, text=True,
                       timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(csrc, 'asan', 'asan_slab_wide_driver')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    assert ' 0 failures' in r.stdout, r.stdout[-1500:]
