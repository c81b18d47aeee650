"""CPU: the host side of IResNet / ContinuousIResNet training on sx_resnet_flow_bwd -- exports, the ctypes record, the coverage
and partial-buffer size functions, the planner on CPU modules, the spectral-norm chain rule, and the host validator under sanitizers."""
import ctypes
import os
import re
import subprocess
import tempfile

import torch
import torch.nn as nn

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.flows.iresnet import spectral_weight_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sx_resnet_bwd_lds_bytes', 'sx_resnet_bwd_partial_floats', 'sx_resnet_flow_bwd')


def _net(dim, widths, act=2, final=0):
    """dim -> widths[0] -> ... (the last width is the output and must equal dim), every layer after the first wrapped."""
    d = _hip.sx_resnet_net()
    ins = [dim] + widths[:-1]
    for i, (o, k) in enumerate(zip(widths, ins)):
        d.layer[i].W, d.layer[i].b = 16, 0
        d.layer[i].out_dim, d.layer[i].in_dim, d.layer[i].sigma_col = o, k, (i - 1 if i >= 1 else -1)
    d.n_layers, d.dim, d.act, d.final_act, d.n_wrapped = len(widths), dim, act, final, max(0, len(widths) - 1)
    return d


def test_entry_points_declared_listed_exported_and_built():
    hdr = open(os.path.join(ROOT, 'include', 'stribor_hip.h')).read()
    declared = set(re.findall(r'\b(sx_[a-z0-9_]+)\s*\(', hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    mk = open(os.path.join(ROOT, 'stribor_amd', 'csrc', 'Makefile')).read()
    assert 'sx_resnet_bwd.hip' in mk and 'asan_resnet_bwd' in mk
    assert '#define SX_ABI_VERSION 3' in hdr and _hip.lib().sx_abi_version() == _hip.SX_ABI_VERSION == 3
    assert re.search(r'#define SX_RESNET_BWD_MAX_WIDTH\s+64', hdr) and _hip.RESNET_BWD_MAX_WIDTH == 64


def test_grads_record_matches_the_header():
    cls = _hip.sx_resnet_grads
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stribor_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %zu\\n", sizeof(sx_resnet_grads), offsetof(sx_resnet_grads, dW), offsetof(sx_resnet_grads, db), '
             'sizeof(((sx_resnet_grads *)0)->dW) / sizeof(float *));', '  return 0;', '}']
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'layout.c')
        with open(src, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), src, '-o', os.path.join(td, 'layout')], check=True)
        out = subprocess.run([os.path.join(td, 'layout')], check=True, capture_output=True, text=True).stdout
    assert [int(v) for v in out.split()] == [ctypes.sizeof(cls), cls.dW.offset, cls.db.offset, _hip.RESNET_MAX_LAYERS]


def test_lds_bytes_over_the_coverage_and_one_step_outside():
    """Forward images (tiles + biases), transposed images (tiles), 4 waves x 2 slots of 1056 floats; 0 outside the coverage."""
    lib = _hip.lib()
    scr = 8 * 1056
    assert lib.sx_resnet_bwd_lds_bytes(_net(3, [3])) == 4 * (1024 + 32 + 1024 + scr)
    assert lib.sx_resnet_bwd_lds_bytes(_net(8, [32, 32, 8])) == 4 * (3 * (1024 + 32) + 3 * 1024 + scr)
    assert lib.sx_resnet_bwd_lds_bytes(_net(33, [48, 33])) == 4 * (2 * (4096 + 64) + 2 * 4096 + scr)
    assert lib.sx_resnet_bwd_lds_bytes(_net(64, [64, 64, 64])) == 4 * (3 * (4096 + 64) + 3 * 4096 + scr) == 132864
    assert lib.sx_resnet_bwd_lds_bytes(_net(20, [16, 40, 24, 20])) == 4 * (12 * 1024 + 64 + 64 + 64 + 32 + 12 * 1024 + scr)
    assert lib.sx_resnet_bwd_lds_bytes(_net(32, [32, 32, 32, 32])) == 4 * (4 * (1024 + 32) + 4 * 1024 + scr)
    for act in range(9):
        assert lib.sx_resnet_bwd_lds_bytes(_net(8, [32, 8], act=act, final=act)) != 0
    # one step outside each bound
    assert lib.sx_resnet_bwd_lds_bytes(_net(65, [32, 65])) == 0
    assert lib.sx_resnet_bwd_lds_bytes(_net(16, [65, 16])) == 0
    assert lib.sx_resnet_bwd_lds_bytes(_net(64, [64, 64, 64, 64])) == 0               # 162 KiB of LDS
    assert lib.sx_resnet_bwd_lds_bytes(_net(8, [32, 8], act=9)) == 0
    assert lib.sx_resnet_bwd_lds_bytes(_net(8, [32, 8], final=9)) == 0
    assert lib.sx_resnet_bwd_lds_bytes(_net(8, [32, 7])) == 0                         # the last layer must map back to dim
    d = _net(8, [32, 8])
    d.n_layers = 5
    assert lib.sx_resnet_bwd_lds_bytes(d) == 0
    assert lib.sx_resnet_lds_bytes(_net(65, [32, 65])) != 0                           # ... which the forward kernel still covers


def test_partial_floats_is_monotone_and_capped():
    lib = _hip.lib()
    d = _net(64, [64, 64, 64])
    per_wave = 12 * 1024 + 6 * 64 + 2 * 6 * 1024
    assert lib.sx_resnet_bwd_partial_floats(d, 0) == 0
    assert lib.sx_resnet_bwd_partial_floats(d, 1) == lib.sx_resnet_bwd_partial_floats(d, 128) == 4 * per_wave
    assert lib.sx_resnet_bwd_partial_floats(d, 129) == 8 * per_wave
    sizes = [lib.sx_resnet_bwd_partial_floats(d, n) for n in range(0, 1 << 17, 1000)]
    assert sizes == sorted(sizes)
    assert lib.sx_resnet_bwd_partial_floats(d, 1 << 40) == lib.sx_resnet_bwd_partial_floats(d, 512 * 128) == 512 * 4 * per_wave
    assert lib.sx_resnet_bwd_partial_floats(_net(65, [32, 65]), 100) == 0


def test_validator_refuses_before_any_launch():
    lib = _hip.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    x, gin, gout, sig = p, p + 4096, p + 8192, p + 12288
    d = _net(64, [64, 64, 64])
    for i in range(3):
        d.layer[i].W = p

    def bad(rc):
        assert rc != 0 and lib.sx_last_error(), rc
    assert lib.sx_resnet_flow_bwd(d, x, None, sig, gin, gout, None, None, None, 0, 100, 1, None) == 0
    bad(lib.sx_resnet_flow_bwd(d, None, None, sig, gin, gout, None, None, None, 4, 1, 1, None))
    bad(lib.sx_resnet_flow_bwd(d, x, None, sig, None, gout, None, None, None, 4, 1, 1, None))
    bad(lib.sx_resnet_flow_bwd(d, x, None, sig, gin, None, None, None, None, 4, 1, 1, None))
    bad(lib.sx_resnet_flow_bwd(d, x + 2, None, sig, gin, gout, None, None, None, 4, 1, 1, None))
    bad(lib.sx_resnet_flow_bwd(d, x, None, sig, gin, gout + 1, None, None, None, 4, 1, 1, None))
    bad(lib.sx_resnet_flow_bwd(d, x, None, sig, gin, gout, None, None, None, 4, -1, 1, None))
    bad(lib.sx_resnet_flow_bwd(d, x, None, None, gin, gout, None, None, None, 4, 1, 1, None))
    assert b'sigma' in lib.sx_last_error()
    g = _hip.sx_resnet_grads()
    g.dW[0] = p
    bad(lib.sx_resnet_flow_bwd(d, x, None, sig, gin, gout, None, None, ctypes.byref(g), 4, 1, 1, None))
    assert b'partial' in lib.sx_last_error()
    bad(lib.sx_resnet_flow_bwd(_net(65, [32, 65]), x, None, sig, gin, gout, None, None, None, 4, 1, 1, None))
    bad(lib.sx_resnet_flow_bwd(_net(64, [64, 64, 64, 64]), x, None, sig, gin, gout, None, None, None, 4, 1, 1, None))


def test_train_plan_on_cpu_modules():
    """Host only: a plan inside the coverage, None outside (those calls compose torch ops)."""
    torch.manual_seed(0)
    inside = [st.IResNet(3, []), st.IResNet(4, [16]), st.ContinuousIResNet(8, [32, 32], time_net=st.net.TimeTanh(8)),
              st.ContinuousIResNet(64, [64, 64], activation='SiLU', time_net=st.net.TimeLog(64)),
              st.ContinuousIResNet(20, [16, 40, 24], activation='GELU', time_net=st.net.TimeTanh(20)),
              st.ContinuousIResNet(33, [48], activation='Tanh', final_activation='Sigmoid', time_net=st.net.TimeFourier(33, 6))]
    for f in inside:
        plan = f._train_plan()
        assert plan is not None and plan[0].dim == f.dim, f
        assert len(f._param_spec()) == 2 * plan[0].n_layers
    outside = [st.IResNet(16, [256]), st.IResNet(16, [32], activation='Hardtanh'), st.IResNet(65, [32]), st.IResNet(16, [65]),
               st.IResNet(64, [64, 64, 64]), st.IResNet(8, [8, 8, 8, 8]), st.IResNet(4, [16]).double()]
    for f in outside:
        assert f._train_plan() is None, f
    assert st.IResNet(65, [32])._kernel_net() is not None           # the no-graph kernel covers it all the same


def test_spectral_weight_grad_matches_autograd():
    torch.manual_seed(1)
    for out_dim, in_dim in ((5, 3), (32, 48), (64, 64)):
        W = torch.randn(out_dim, in_dim, dtype=torch.float64, requires_grad=True)
        u = nn.functional.normalize(torch.randn(out_dim, dtype=torch.float64), dim=0)
        v = nn.functional.normalize(torch.randn(in_dim, dtype=torch.float64), dim=0)
        G = torch.randn(out_dim, in_dim, dtype=torch.float64)
        sigma = torch.dot(u, W.mv(v))
        ((W / sigma) * G).sum().backward()
        got = spectral_weight_grad(G, W.detach(), u, v, sigma.detach())
        assert torch.allclose(got, W.grad, rtol=1e-12, atol=1e-12)


def test_validator_under_address_and_ub_sanitizers():
    """`make asan_resnet_bwd`: the library's host code (--offload-host-only, -fsanitize=address,undefined) linked with
    tests/asan_resnet_bwd_driver.cpp, a stand-alone program that drives the two size functions and the validator without a GPU."""
    csrc = os.path.join(ROOT, 'stribor_amd', 'csrc')
    b = subprocess.run(['make', '-C', csrc, '-j', str(min(8, os.cpu_count() or 1)), 'asan_resnet_bwd'], capture_output=True, text=True,
                       timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(csrc, 'asan', 'asan_resnet_bwd_driver')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    assert ' 0 failures' in r.stdout, r.stdout[-1500:]
