"""CPU: the host side of EquivariantNet on sx_equivariant_fwd / sx_equivariant_bwd -- the closed-form backward the kernel is written
from against autograd in fp64, the composed path on CPU tensors, the planner's table (host code: shapes and the library's LDS sizes,
so the device may be the CPU), the exports, DiffeqDeepset's route and the host validators under sanitizers."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest
import torch
import torch.nn as nn

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.net.equivariant import EquivariantLayer, EquivariantNet, equivariant_backward_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sx_equivariant_lds_bytes', 'sx_equivariant_bwd_partial_floats', 'sx_equivariant_fwd', 'sx_equivariant_bwd')
CPU = torch.device('cpu')


def _mask(kind, B, N, g):
    if kind == 'none':
        return None
    if kind == 'binary':
        m = (torch.rand(B, N, 1, generator=g) < 0.6).double()
        m[:, 0] = 1.0                                        # at least one element kept per set
        return m
    return 0.25 + torch.rand(B, N, 1, generator=g, dtype=torch.float64)


@pytest.mark.parametrize('hidden,N,mask_kind,act,final', [
    (h, n, m, a, f) for (h, n, m), (a, f) in itertools.product(
        itertools.product(([6], [6, 7]), (1, 5), ('none', 'binary', 'fractional')), (('Tanh', None), ('Sigmoid', 'Softplus'), ('Sigmoid', 'Tanh')))],
    ids=lambda v: str(v))
def test_closed_form_backward_matches_autograd_in_fp64(hidden, N, mask_kind, act, final):
    g = torch.Generator().manual_seed(len(hidden) * 100 + N)
    torch.manual_seed(7)
    net = EquivariantNet(4, hidden, 3, activation=act, final_activation=final).double()
    B = 3
    x = torch.randn(B, N, 4, generator=g, dtype=torch.float64, requires_grad=True)
    mask = _mask(mask_kind, B, N, g)
    gy = torch.randn(B, N, 3, generator=g, dtype=torch.float64)
    params = [p for l in net.layers for p in (l.l1.weight, l.l1.bias, l.l2.weight, l.l2.bias)]
    want = torch.autograd.grad(net.forward_twice_differentiable(x, mask=mask), [x] + params, gy)
    dx, grads = equivariant_backward_closed_form(net.layers, net.activation, net.final_activation, x.detach(), mask, gy)
    got = [dx] + [t for layer in grads for t in layer]
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        rel = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
        assert rel <= 1e-10, (i, rel)


@pytest.mark.parametrize('masked', [False, True])
def test_cpu_forward_is_the_composed_sequence_bit_for_bit(masked):
    torch.manual_seed(3)
    net = EquivariantNet(5, [9, 8], 4, final_activation='Sigmoid')
    x = torch.randn(2, 7, 5)
    mask = (torch.rand(2, 7, 1) < 0.7).float() if masked else None
    assert net._last_path is None
    y = net(x, mask=mask)
    assert net._last_path == 'composed'
    assert torch.equal(y, net.forward_twice_differentiable(x, mask=mask))
    h = x
    for layer in net.layers[:-1]:
        h = net.activation(layer(h, mask=mask))
    assert torch.equal(y, net.final_activation(net.layers[-1](h, mask=mask)))
    # a graph on the CPU: composed, differentiable twice
    x.requires_grad_(True)
    g1 = torch.autograd.grad(net(x, mask=mask).sum(), x, create_graph=True)[0]
    assert torch.autograd.grad(g1.sum(), x)[0].shape == x.shape


class _Sub(EquivariantNet):
    pass


def _no_l2_bias():
    net = EquivariantNet(4, [8], 3)
    net.layers[0].l2 = nn.Linear(4, 8, bias=False)
    return net


def _elu2():
    net = EquivariantNet(4, [8], 3, activation='ELU')
    net.activation = nn.ELU(alpha=2.0)
    return net


# (the net, the input's shape, a graph wanted) -> covered?  Literals: the coverage of DESIGN.md section 4.16.
PLANS = [
    ('widest', lambda: EquivariantNet(64, [64, 64], 128), (2, 128, 64), False, True),
    ('n129', lambda: EquivariantNet(64, [64, 64], 128), (2, 129, 64), False, False),
    ('in65', lambda: EquivariantNet(65, [64, 64], 128), (2, 128, 65), False, False),
    ('hidden65', lambda: EquivariantNet(64, [64, 65], 128), (2, 128, 64), False, False),
    ('out129', lambda: EquivariantNet(64, [64, 64], 129), (2, 128, 64), False, False),
    ('three_hidden', lambda: EquivariantNet(4, [8, 8, 8], 3), (2, 5, 4), False, False),
    ('no_hidden', lambda: EquivariantNet(4, [], 3), (2, 5, 4), False, False),
    ('subclass', lambda: _Sub(4, [8], 3), (2, 5, 4), False, False),
    ('no_l2_bias', _no_l2_bias, (2, 5, 4), False, False),
    ('elu2', _elu2, (2, 5, 4), False, False),
    ('silu', lambda: EquivariantNet(4, [8], 3, activation='SiLU'), (2, 5, 4), False, False),
    ('final_gelu', lambda: EquivariantNet(4, [8], 3, final_activation='GELU'), (2, 5, 4), False, False),
    ('final_softplus', lambda: EquivariantNet(4, [8], 3, activation='LeakyReLU', final_activation='Softplus'), (2, 5, 4), False, True),
    ('one_set', lambda: EquivariantNet(4, [8], 3), (5, 4), False, True),
    ('one_row', lambda: EquivariantNet(4, [8], 3), (4,), False, False),
    ('empty', lambda: EquivariantNet(4, [8], 3), (0, 5, 4), False, False),
    ('wrong_width', lambda: EquivariantNet(4, [8], 3), (2, 5, 6), False, False),
    # the backward's narrower edges: in <= 32, out <= 64, two hidden layers of <= 32 units, or one of <= 64 with out <= 32
    ('bwd_edge', lambda: EquivariantNet(32, [32, 32], 64), (2, 128, 32), True, True),
    ('bwd_one64', lambda: EquivariantNet(32, [64], 32), (2, 128, 32), True, True),
    ('bwd_in33', lambda: EquivariantNet(33, [32, 32], 64), (2, 128, 33), True, False),
    ('bwd_in33_no_graph', lambda: EquivariantNet(33, [32, 32], 64), (2, 128, 33), False, True),
    ('bwd_out65', lambda: EquivariantNet(32, [32, 32], 65), (2, 128, 32), True, False),
    ('bwd_hidden33', lambda: EquivariantNet(32, [33, 32], 64), (2, 128, 32), True, False),
    ('bwd_hidden_32_33', lambda: EquivariantNet(32, [32, 33], 32), (2, 128, 32), True, False),
    ('bwd_one64_out33', lambda: EquivariantNet(32, [64], 33), (2, 128, 32), True, False),
    ('bwd_one65', lambda: EquivariantNet(32, [65], 32), (2, 128, 32), True, False),
    ('bwd_widest', lambda: EquivariantNet(64, [64, 64], 128), (2, 128, 64), True, False),
]


def _descriptor(net, shape):
    params = [p for l in net.layers for p in (l.l1.weight, l.l1.bias, l.l2.weight, l.l2.bias)]
    d = _hip.sx_equivariant_net()
    for l, layer in enumerate(net.layers[:3]):
        d.A[l], d.a[l], d.B[l], d.b[l] = (t.data_ptr() for t in params[4 * l:4 * l + 4])
        d.out_dim[l] = layer.l1.out_features
    d.n_layers, d.in_dim, d.set_size = len(net.layers), shape[-1], shape[-2]
    d.act = _hip.ACT_CODES[type(net.activation).__name__]
    d.final_act = _hip.ACT_CODES[type(net.final_activation).__name__]
    return d


@pytest.mark.parametrize('row', PLANS, ids=lambda r: r[0])
def test_planner_table(row):
    _, make, shape, graph, covered = row
    torch.manual_seed(0)
    net = make()
    plan = net.kernel_plan(torch.Size(shape), graph, CPU)
    assert (plan is not None) == covered
    if covered:
        params, dims, act, fact = plan
        assert len(params) == 4 * len(net.layers) and dims[0] == shape[-1] and dims[-1] == net.layers[-1].l1.out_features
        assert act == _hip.ACT_CODES[type(net.activation).__name__] and fact == _hip.ACT_CODES[type(net.final_activation).__name__]


def test_planner_declines_parameters_it_cannot_read_in_place():
    torch.manual_seed(0)
    net = EquivariantNet(4, [8], 3)
    assert net.kernel_plan(torch.Size((2, 5, 4)), False, CPU) is not None
    assert net.kernel_plan(torch.Size((2, 5, 4)), False, torch.device('cuda', 0)) is None       # the parameters live elsewhere
    assert net.double().kernel_plan(torch.Size((2, 5, 4)), False, CPU) is None


SHAPE_ONLY = ('widest', 'n129', 'in65', 'hidden65', 'out129', 'three_hidden', 'no_hidden', 'final_softplus', 'bwd_edge', 'bwd_one64',
              'bwd_in33', 'bwd_out65', 'bwd_hidden33', 'bwd_hidden_32_33', 'bwd_one64_out33', 'bwd_one65', 'bwd_widest')


@pytest.mark.parametrize('row', [r for r in PLANS if r[0] in SHAPE_ONLY], ids=lambda r: r[0])
def test_lds_bytes_is_nonzero_exactly_where_the_planner_covers(row):
    _, make, shape, graph, covered = row
    torch.manual_seed(0)
    net = make()
    d = _descriptor(net, shape)
    lib = _hip.lib()
    fwd, bwd = lib.sx_equivariant_lds_bytes(ctypes.byref(d), 0), lib.sx_equivariant_lds_bytes(ctypes.byref(d), 1)
    assert fwd <= _hip.CNF_LDS_BYTES and bwd <= _hip.CNF_LDS_BYTES
    assert ((bwd if graph else fwd) != 0) == covered
    assert bwd == 0 or fwd != 0                       # the backward's coverage lies inside the forward's
    assert (lib.sx_equivariant_bwd_partial_floats(ctypes.byref(d), shape[0] * shape[1]) != 0) or bwd == 0


def test_entry_points_declared_listed_exported_and_built():
    hdr = open(os.path.join(ROOT, 'include', 'stribor_hip.h')).read()
    declared = set(re.findall(r'\b(sx_[a-z0-9_]+)\s*\(', hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    mk = open(os.path.join(ROOT, 'stribor_amd', 'csrc', 'Makefile')).read()
    assert 'sx_equivariant.hip' in mk and 'asan_equivariant' in mk
    for name, value in (('SIZE', 128), ('IN', 64), ('HIDDEN', 64), ('OUT', 128), ('BWD_MAX_IN', 32), ('BWD_MAX_HIDDEN', 64), ('BWD_MAX_OUT', 64)):
        macro = 'SX_EQUIVARIANT_' + (name if name.startswith('BWD') else 'MAX_' + name)
        assert re.search(r'#define %s\s+%d\b' % (macro, value), hdr), macro
        assert getattr(_hip, macro[3:]) == value


def test_records_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stribor_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sx_equivariant_net), offsetof(sx_equivariant_net, a), '
             'offsetof(sx_equivariant_net, B), offsetof(sx_equivariant_net, b), offsetof(sx_equivariant_net, n_layers), '
             'offsetof(sx_equivariant_net, set_size), offsetof(sx_equivariant_net, out_dim), sizeof(sx_equivariant_grads), '
             'offsetof(sx_equivariant_grads, db));', '  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'layout')], check=True)
    out = subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout
    n, g = _hip.sx_equivariant_net, _hip.sx_equivariant_grads
    assert [int(v) for v in out.split()] == [ctypes.sizeof(n), n.a.offset, n.B.offset, n.b.offset, n.n_layers.offset, n.set_size.offset,
                                             n.out_dim.offset, ctypes.sizeof(g), g.db.offset]


@pytest.mark.parametrize('grad', [False, True])
def test_diffeq_deepset_takes_the_twice_differentiable_path_in_every_grad_mode(monkeypatch, grad):
    torch.manual_seed(1)
    f = st.net.DiffeqDeepset(3 + 1, [8], 3)
    calls = {'twice': 0, 'forward': 0}
    twice = EquivariantNet.forward_twice_differentiable

    def count_twice(self, *a, **k):
        calls['twice'] += 1
        return twice(self, *a, **k)

    monkeypatch.setattr(EquivariantNet, 'forward_twice_differentiable', count_twice)
    x = torch.randn(2, 5, 3)
    mask = torch.ones(2, 5, 1)
    with torch.set_grad_enabled(grad):
        y = f(torch.tensor(0.5), x, mask=mask)
    assert calls['twice'] == 1 and f.net._last_path is None
    h = torch.cat([torch.ones_like(x[..., :1]) * 0.5, x], -1)
    assert torch.equal(y, twice(f.net, h, mask=mask))
    # a subclass that brings its own forward keeps it
    class Own(EquivariantNet):
        def forward(self, x, mask=None, **kwargs):
            calls['forward'] += 1
            return super().forward_twice_differentiable(x, mask=mask)
    g = st.net.DiffeqConcat(Own(4, [8], 3))
    with torch.set_grad_enabled(grad):
        g(torch.tensor(0.5), x)
    assert calls['forward'] == 1 and calls['twice'] == 2


def test_validators_under_address_and_ub_sanitizers():
    """`make asan_equivariant`: the library's host code (--offload-host-only, -fsanitize=address,undefined) linked with
    tests/asan_equivariant_driver.cpp, a stand-alone program that drives the size functions and both validators without a GPU."""
    csrc = os.path.join(ROOT, 'stribor_amd', 'csrc')
    b = subprocess.run(['make', '-C', csrc, '-j', str(min(8, os.cpu_count() or 1)), 'asan_equivariant'], capture_output=True, text=True,
                       timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(csrc, 'asan', 'asan_equivariant_driver')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    assert ' 0 failures' in r.stdout, r.stdout[-1500:]
