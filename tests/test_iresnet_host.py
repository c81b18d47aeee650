"""Host (no GPU): the IResNet / ContinuousIResNet surface (stribor/flows/iresnet.py) against fixture F14
(tests/golden/make_golden_iresnet.py) -- constructors, state_dict keys and shapes, the reference's init stream draw for draw --
and the C ABI of sx_resnet_flow / sx_spectral_sigma."""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import flowdesc as fd
from goldens import Golden

import stribor_amd as st
from stribor_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def test_exported_from_the_package():
    assert st.IResNet is st.flows.IResNet and st.ContinuousIResNet is st.flows.ContinuousIResNet
    assert issubclass(st.IResNet, st.Transform) and issubclass(st.ContinuousIResNet, st.Transform)


def test_constructor_surface_and_state_keys_match_f14():
    g = Golden('f14_iresnet')
    cases = [c for c in g.meta if c.startswith('grid/')]
    assert len(cases) == 24
    for case in cases:
        d = g.meta[case]['desc']
        f = fd.build_transform(st, d)
        want = g.state(case)
        got = f.state_dict()
        assert list(got) == list(want) or set(got) == set(want), (case, sorted(set(got) ^ set(want)))
        for k, v in want.items():
            assert tuple(got[k].shape) == tuple(v.shape), (case, k)
        f.load_state_dict(want)
        n_lin = len(d['hidden']) + 1
        assert f'net.net.0.weight' in got and 'net.net.0.weight_orig' not in got      # mlp.py:46: the first Linear is not wrapped
        for i in range(1, n_lin):
            for suffix in ('weight_orig', 'weight_u', 'weight_v', 'bias'):
                assert f'net.net.{2 * i}.{suffix}' in got
        assert torch.count_nonzero(want[f'net.net.{2 * (n_lin - 1)}.bias']) == 0       # mlp.py:53
    f = st.ContinuousIResNet(3, [7], activation='Tanh', final_activation='Sigmoid', time_net=st.net.TimeTanh(3), n_power_iterations=2)
    assert f.net.net[2]._forward_pre_hooks and isinstance(f.net.net[-1], torch.nn.Sigmoid)
    with pytest.raises(TypeError):
        st.ContinuousIResNet(3, [7], 'ReLU')                 # keyword-only after hidden_dims (iresnet.py:66-74)
    assert st.IResNet(2, []).log_det_jacobian(torch.zeros(1, 2), torch.zeros(1, 2)) is NotImplementedError


def test_default_init_matches_reference_rng_stream():
    """Same seed -> bit-identical default state (Linear weights, biases, spectral-norm u / v, time-net parameters)."""
    g = Golden('f14_iresnet')
    seeds = g.meta['seeds']
    for case, want in seeds['state_sha256'].items():
        torch.manual_seed(seeds['seed'])
        f = fd.build_transform(st, g.meta[case]['desc'])
        got = {k: _sha(v) for k, v in f.state_dict().items()}
        assert got == want, (case, [k for k in want if got.get(k) != want[k]])
    w = Golden('f14_iresnet_wide')
    for case, m in w.meta.items():
        torch.manual_seed(m['seed'])
        f = fd.build_transform(st, m['desc'])
        assert {k: _sha(v) for k, v in f.state_dict().items()} == m['state_sha256'], case


def test_neural_flow_from_the_reference_test_builds():
    """test_neural_flow.py:9-21 restated: the mixed stack constructs and holds the reference's state."""
    g = Golden('f14_iresnet')
    m = g.meta['neural_flow']
    torch.manual_seed(123)
    nf = st.NeuralFlow([fd.build_transform(st, d) for d in m['desc']])
    want = g.state('neural_flow')
    got = nf.state_dict()
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v), k


def test_new_entry_points_exported():
    for name in ('sx_resnet_flow', 'sx_spectral_sigma', 'sx_resnet_lds_bytes'):
        assert name in _hip.EXPORTS
        assert hasattr(_hip.lib(), name)


def test_resnet_structs_match_the_header():
    structs = {'sx_resnet_layer': _hip.sx_resnet_layer, 'sx_resnet_net': _hip.sx_resnet_net, 'sx_sn_layer': _hip.sx_sn_layer,
               'sx_sn_job': _hip.sx_sn_job}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stribor_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append('  printf("%s %%zu", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            lines.append('  printf(" %%zu", offsetof(%s, %s));' % (name, field))
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}']
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, 'layout.c')
        with open(src, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), src, '-o', os.path.join(td, 'layout')], check=True)
        out = subprocess.run([os.path.join(td, 'layout')], check=True, capture_output=True, text=True).stdout
    seen = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out.strip().splitlines()}
    for name, cls in structs.items():
        assert seen[name] == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], name


def _net(dim, widths, wrapped_from=1):
    d = _hip.sx_resnet_net()
    ins = [dim] + widths[:-1]
    for i, (o, k) in enumerate(zip(widths, ins)):
        d.layer[i].W, d.layer[i].b = 16, 0
        d.layer[i].out_dim, d.layer[i].in_dim, d.layer[i].sigma_col = o, k, (i - wrapped_from if i >= wrapped_from else -1)
    d.n_layers, d.dim, d.act, d.final_act, d.n_wrapped = len(widths), dim, 2, 0, max(0, len(widths) - wrapped_from)
    return d


def test_lds_budget_and_argument_checks():
    """The LDS image (tiles of 32 padded to 1, 2 or 4) and the launcher's refusals -- all decided on the host, no launch."""
    lib = _hip.lib()
    assert lib.sx_resnet_lds_bytes(_net(64, [64, 64, 64])) == 4 * 3 * (2 * 2 * 1024 + 2 * 32)
    assert lib.sx_resnet_lds_bytes(_net(128, [128, 128])) == 4 * 2 * (4 * 4 * 1024 + 4 * 32)
    assert lib.sx_resnet_lds_bytes(_net(128, [128, 128, 128])) > _hip.RESNET_LDS_BYTES
    assert lib.sx_resnet_lds_bytes(_net(2, [2], wrapped_from=5)) == 4 * (1024 + 32)
    p = ctypes.c_void_p(16)
    sig = ctypes.c_void_p(16)
    # too wide for the LDS budget
    assert lib.sx_resnet_flow(ctypes.byref(_net(128, [128, 128, 128])), p, p, 4, None, None, -1, None, None, 0, sig, 1, 3, 1, None) < 0
    # the last layer must map back to dim, sigma needs `iterations` rows, time nets need t
    assert lib.sx_resnet_flow(ctypes.byref(_net(64, [64, 32])), p, p, 4, None, None, -1, None, None, 0, sig, 1, 3, 1, None) < 0
    assert lib.sx_resnet_flow(ctypes.byref(_net(64, [64, 64])), p, p, 4, None, None, -1, None, None, 0, sig, 2, 3, 1, None) < 0
    assert lib.sx_resnet_flow(ctypes.byref(_net(64, [64, 64])), p, p, 4, None, None, 2, p, None, 0, sig, 1, 3, 1, None) < 0
    assert lib.sx_resnet_flow(ctypes.byref(_net(200, [64, 200])), p, p, 4, None, None, -1, None, None, 0, sig, 1, 3, 1, None) < 0
    job = _hip.sx_sn_job()
    job.n_layers = 1
    job.layer[0].W = job.layer[0].u = job.layer[0].v = 16
    job.layer[0].out_dim, job.layer[0].in_dim, job.layer[0].n_power, job.layer[0].eps = 256, 64, 1, 1e-12
    assert lib.sx_spectral_sigma(ctypes.byref(job), 1, sig, None) < 0        # wider than 128
    assert lib.sx_spectral_sigma(ctypes.byref(job), 0, sig, None) < 0


def test_cpu_tensors_are_refused():
    f = st.IResNet(2, [8])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        f(torch.randn(3, 2))
