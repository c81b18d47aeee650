"""CPU: the host side of training ContinuousAffineCoupling on sx_time_coupling_bwd -- the closed-form backward the kernel is written
from against fp64 autograd of the oracle, the planner's gate and the library's size function (host code: the device may be the CPU),
the exports and the record layout, and the host validator under sanitizers (a stand-alone program)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.flows.coupling import time_coupling_closed_form

import timecouplinghelp as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sx_time_coupling_bwd_lds_bytes', 'sx_time_coupling_bwd_partial_floats', 'sx_time_coupling_bwd')
CPU = torch.device('cpu')

# (D, H, L, time kind, half-width, concatenate_time, activation, mask): every time kind at both half-widths, without the time
# column, latent 0 and 3, the three masks and 'none' at D = 1, the seven activations
CASES = [(6, 9, 0, 'identity', 6, True, 'Tanh', 'ordered_left_half'), (6, 9, 3, 'identity', 1, True, 'ReLU', 'parity_odd'),
         (6, 9, 3, 'linear', 6, True, 'Sigmoid', 'random_half'), (5, 7, 0, 'linear', 1, False, 'ELU', 'parity_odd'),
         (6, 9, 0, 'tanh', 6, False, 'Softplus', 'random_half'), (5, 7, 3, 'tanh', 1, True, 'LeakyReLU', 'ordered_left_half'),
         (6, 9, 3, 'log', 6, True, 'Identity', 'parity_odd'), (5, 7, 0, 'log', 1, True, 'Tanh', 'random_half'),
         (1, 8, 2, 'tanh', 1, True, 'Tanh', 'none'), (1, 8, 0, 'log', 1, False, 'Sigmoid', 'none'),
         (7, 5, 3, 'tanh', 7, True, 'ELU', 'none')]


@pytest.mark.parametrize('mode', sorted(th.MODES))
@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(map(str, c)))
def test_closed_form_backward_matches_autograd_of_the_oracle_in_fp64(monkeypatch, case, mode):
    """time_coupling_closed_form (the formulas sx_time_coupling_bwd implements) in fp64 against autograd of
    oracle.continuous_affine_coupling: gx, gt, glatent, the four weight gradients and the scale gradient within
    1e-12 * max(1, max |truth|).  Both directions, sigma = +-1 with a non-zero cotangent on the log-det."""
    D, H, L, kind, half, concat, act, mask = case
    f = th.make_layer(D, H, L, kind, half, concat, act, mask, seed=3)
    th.oracle_masks(monkeypatch, [f], D)
    reverse, sigma, uses = th.MODES[mode]
    x, t, lat, wy, wl = th.inputs(37, D, L, seed=11)
    want = th.truth(f, mode, x, t, lat, wy, wl)
    p = {k: v.detach().double() for k, v in f.named_parameters()}
    got = time_coupling_closed_form(x.double(), t.double(), None if lat is None else lat.double(), p['latent_net.net.0.weight'],
                                    p['latent_net.net.0.bias'], p['latent_net.net.2.weight'], p['latent_net.net.2.bias'],
                                    p.get('time_net.scale'), torch.from_numpy(f.mask_vector(D)), act, f.time_net.kind, concat, reverse,
                                    sigma, gy=wy.double(), gl=wl.double() if uses else None)
    pairs = [('gx', 'x'), ('gt', 't'), ('glatent', 'latent'), ('dW1', 'latent_net.net.0.weight'), ('db1', 'latent_net.net.0.bias'),
             ('dW2', 'latent_net.net.2.weight'), ('db2', 'latent_net.net.2.bias'), ('dscale', 'time_net.scale')]
    for mine, theirs in pairs:
        ref = want.get(theirs)
        if ref is None:
            assert got[mine] is None, mine
            continue
        err = (got[mine].reshape(ref.shape) - ref).abs().max().item()
        assert err <= 1e-12 * max(1.0, ref.abs().max().item()), (mine, err)
    # the live rows of W2 alone carry a gradient, and only the conditioning columns of W1
    m = torch.from_numpy(f.mask_vector(D)) > 0.5
    assert (got['dW2'][:D][m] == 0).all() and (got['dW2'][D:][m] == 0).all()
    assert (got['dW1'][:, :D][:, ~m] == 0).all()


def _desc(D=4, L=0, H=16, mask=0x3, act=1, kind=2, half=None, concat=1):
    d = _hip.sx_time_coupling_net()
    d.dim, d.latent_dim, d.hidden, d.act, d.time_kind, d.time_half, d.concat_time = D, L, H, act, kind, D if half is None else half, concat
    d.mask[0], d.mask[1] = mask & 0xffffffff, mask >> 32
    return d


GATE = [  # (tag, make_layer arguments, covered)
    ('small', dict(D=4, H=16, L=0), True), ('latent', dict(D=4, H=16, L=3), True), ('odd', dict(D=33, H=40, L=5, mask='parity_odd'), True),
    ('widest', dict(D=64, H=64, L=0), True), ('none-64', dict(D=64, H=64, L=0, mask='none'), True),
    ('dim-1', dict(D=1, H=8, L=2, mask='none', half=1), True), ('in-64', dict(D=40, H=8, L=24, mask='random_half'), True),
    ('identity', dict(D=4, H=16, L=0, kind='identity'), True), ('half-1', dict(D=4, H=16, L=0, kind='log', half=1), True),
    ('no-time-column', dict(D=4, H=16, L=0, concat=False), True),
    ('H-65', dict(D=4, H=65, L=0), False), ('D-65', dict(D=65, H=16, L=0), False), ('D+L-65', dict(D=33, H=16, L=32), False),
    ('two-hidden', dict(D=4, H=16, L=0, hidden=[16, 16]), False), ('SiLU', dict(D=4, H=16, L=0, act='SiLU'), False),
    ('GELU', dict(D=4, H=16, L=0, act='GELU'), False), ('dim-1-kept', dict(D=1, H=8, L=2, mask='parity_odd', half=1), False)]


@pytest.mark.parametrize('row', GATE, ids=lambda r: r[0])
def test_planner_and_lds_bytes_agree_on_the_coverage(row):
    tag, kw, covered = row
    f = th.make_layer(**kw)
    D, L = kw['D'], kw['L']
    plan = f._train_plan(D, L, CPU)
    assert (plan is not None) == covered, tag
    if covered:
        d, keep = plan
        assert 0 < _hip.lib().sx_time_coupling_bwd_lds_bytes(d) <= _hip.CNF_LDS_BYTES
        assert _hip.lib().sx_time_coupling_bwd_partial_floats(d, 300) > 0
        assert (d.dim, d.latent_dim, d.hidden, d.concat_time) == (D, L, kw['H'], int(kw.get('concat', True)))
        assert all(ctypes.cast(getattr(d, n), ctypes.c_void_p).value == p.data_ptr() for n, p in zip(('W1', 'b1', 'W2', 'b2'), keep))


@pytest.mark.parametrize('how', ['fourier', 'hand-net', 'own-time-net', 'final-activation', 'leaky-slope', 'fp64'])
def test_planner_declines_what_the_kernel_cannot_read(how):
    D = 4
    f = th.make_layer(D, 16, 0)
    if how == 'fourier':
        f = st.ContinuousAffineCoupling(st.net.MLP(D + 1, [16], 2 * D), st.net.TimeFourier(2 * D, 5), 'ordered_left_half')
    elif how == 'hand-net':
        from stribor_amd.util.flowdesc import HandNet
        f = st.ContinuousAffineCoupling(HandNet(D + 1, 16, 2 * D), st.net.TimeTanh(2 * D), 'ordered_left_half')
    elif how == 'own-time-net':
        class Own(st.net.TimeTanh):
            def forward(self, t):
                return super().forward(t) * 0.5
        f = st.ContinuousAffineCoupling(st.net.MLP(D + 1, [16], 2 * D), Own(2 * D), 'ordered_left_half')
    elif how == 'final-activation':
        f = st.ContinuousAffineCoupling(st.net.MLP(D + 1, [16], 2 * D, final_activation='Tanh'), st.net.TimeTanh(2 * D), 'ordered_left_half')
    elif how == 'leaky-slope':
        f = st.ContinuousAffineCoupling(st.net.MLP(D + 1, [16], 2 * D, activation=torch.nn.LeakyReLU(0.2)), st.net.TimeTanh(2 * D),
                                        'ordered_left_half')
    else:
        f = f.double()
    assert f._train_plan(D, 0, CPU) is None
    assert th.make_layer(D, 16, 0)._train_plan(D, 0, CPU) is not None


def test_lds_bytes_gate_on_the_integer_fields():
    lib = _hip.lib()
    assert lib.sx_time_coupling_bwd_lds_bytes(_desc()) > 0                  # (every pointer is NULL: the integer fields alone are read)
    assert lib.sx_time_coupling_bwd_lds_bytes(_desc(D=64, H=64, mask=0xffffffff)) > 0
    assert lib.sx_time_coupling_bwd_lds_bytes(_desc(D=64, H=64, mask=0)) <= _hip.CNF_LDS_BYTES
    for bad in (_desc(H=65), _desc(D=65, mask=0xffffffff), _desc(D=33, L=32, mask=0xffff), _desc(act=7), _desc(act=8), _desc(kind=4),
                _desc(half=2), _desc(mask=0xf), _desc(mask=0x13), _desc(D=1, mask=1), _desc(concat=2), _desc(H=0), _desc(L=-1)):
        assert lib.sx_time_coupling_bwd_lds_bytes(bad) == 0
        assert lib.sx_time_coupling_bwd_partial_floats(bad, 128) == 0
    assert lib.sx_time_coupling_bwd_partial_floats(_desc(), 0) == 0


def test_entry_points_declared_listed_exported_and_built():
    hdr = open(os.path.join(ROOT, 'include', 'stribor_hip.h')).read()
    declared = set(re.findall(r'\b(sx_[a-z0-9_]+)\s*\(', hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    mk = open(os.path.join(ROOT, 'stribor_amd', 'csrc', 'Makefile')).read()
    assert 'sx_time_coupling_bwd.hip' in mk and 'asan_time_coupling' in mk
    assert re.search(r'sx_time_coupling_bwd\.o: FLAGS \+= -ffp-contract=off -fno-slp-vectorize', mk)
    for name in ('DIM', 'IN', 'HIDDEN'):
        assert re.search(r'#define SX_TIME_COUPLING_BWD_MAX_%s\s+64\b' % name, hdr), name
        assert getattr(_hip, 'TIME_COUPLING_BWD_MAX_' + name) == 64
    assert _hip.lib().sx_abi_version() == 3 and re.search(r'#define SX_ABI_VERSION\s+3\b', hdr)


def test_records_match_the_header(tmp_path):
    """Size and every field offset of the two records, as gcc lays them out from the header, against the ctypes mirrors."""
    structs = {'sx_time_coupling_net': _hip.sx_time_coupling_net, 'sx_time_coupling_grads': _hip.sx_time_coupling_grads}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stribor_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append('  printf("%%zu", sizeof(%s));' % name)
        lines += ['  printf(" %%zu", offsetof(%s, %s));' % (name, field) for field, _ in cls._fields_]
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'layout')], check=True)
    out = subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line, cls in zip(out, structs.values()):
        assert [int(v) for v in line.split()] == [ctypes.sizeof(cls)] + [getattr(cls, field).offset for field, _ in cls._fields_], cls


def test_validator_under_address_and_ub_sanitizers():
    """`make asan_time_coupling`: the library's host code (--offload-host-only, -fsanitize=address,undefined) linked with
    tests/asan_time_coupling_driver.cpp, a stand-alone program that drives the size functions and the validator without a GPU."""
    csrc = os.path.join(ROOT, 'stribor_amd', 'csrc')
    b = subprocess.run(['make', '-C', csrc, '-j', str(min(8, os.cpu_count() or 1)), 'asan_time_coupling'], capture_output=True, text=True,
                       timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(csrc, 'asan', 'asan_time_coupling_driver')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    assert ' 0 failures' in r.stdout, r.stdout[-1500:]
