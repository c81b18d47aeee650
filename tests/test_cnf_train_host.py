"""CPU: the host side of CNF training on the kernels -- the new entry points, their validators at every coverage edge, and the torch
restatement of one evaluation (value, Hutchinson estimate and their adjoints) against reverse mode applied twice, in fp64."""
import ctypes
import os
import re

import pytest
import torch

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.flows import cnf

import cnftrainhelp as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sx_cnf_train_lds_bytes', 'sx_cnf_train_partial_floats', 'sx_cnf_train_fwd', 'sx_cnf_train_bwd')


def test_new_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'stribor_hip.h')).read()
    declared = set(re.findall(r'\b(sx_[a-z0-9_]+)\s*\(', hdr))
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert _hip.lib().sx_abi_version() == 3          # (the change only adds symbols)


def _net(dim, hidden, latent=0, act=1):
    """An sx_cnf_net with the integer fields of this shape (the validators test the weight pointers for NULL only)."""
    d = _hip.sx_cnf_net()
    widths = [1 + dim + latent] + list(hidden) + [dim]
    for i in range(min(3, len(widths) - 1)):          # (the struct holds three layers; a fourth only shows in n_layers)
        d.layer[i].W, d.layer[i].b = 64, 64
        d.layer[i].out_dim, d.layer[i].in_dim = widths[i + 1], widths[i]
    d.n_layers, d.dim, d.latent_dim, d.act = len(widths) - 1, dim, latent, act
    return d


INSIDE = [(3, [5], 0), (32, [32], 0), (6, [32, 24], 2), (5, [32, 32], 58), (1, [1], 0), (2, [8], 61)]
# (hidden 33 .. 64: the two-tile adjoint sweep does not build without scratch, DESIGN.md "CNF training")
OUTSIDE = [(3, [65], 0), (3, [33], 0), (3, [64, 64], 0), (33, [16], 0), (5, [16], 59), (3, [16, 16, 16], 0), (0, [8], 0)]


@pytest.mark.parametrize('shape', INSIDE)
def test_validators_inside_the_coverage(shape):
    lib = _hip.lib()
    d = _net(*shape)
    fwd, bwd = lib.sx_cnf_train_lds_bytes(d, 0), lib.sx_cnf_train_lds_bytes(d, 1)
    assert 0 < fwd < bwd <= _hip.CNF_LDS_BYTES
    one, two = lib.sx_cnf_train_partial_floats(d, 128), lib.sx_cnf_train_partial_floats(d, 130)
    assert one > 0 and two == 2 * one                         # one partial per wave, four waves per 128 rows
    assert lib.sx_cnf_train_partial_floats(d, 10 ** 9) == 512 * one          # (capped: the partials do not grow with the batch)
    assert lib.sx_cnf_train_partial_floats(d, -1) == 0


@pytest.mark.parametrize('shape', OUTSIDE)
def test_validators_outside_the_coverage(shape):
    lib = _hip.lib()
    d = _net(*shape)
    assert lib.sx_cnf_train_lds_bytes(d, 0) == 0 and lib.sx_cnf_train_lds_bytes(d, 1) == 0
    assert lib.sx_cnf_train_partial_floats(d, 100) == 0
    # the entry points refuse before they launch (no device is touched: this runs without a GPU)
    g = _hip.sx_cnf_train_grads()
    assert lib.sx_cnf_train_fwd(d, 64, None, 64, 64, 64, None, 4, 2, 1, 0.0, 1.0, 0.0, None) != 0
    assert lib.sx_cnf_train_bwd(d, 64, None, 64, 64, 64, 64, None, 64, g, 4, 2, 1, 0.0, 1.0, 0.0, None) != 0


def test_activation_and_per_call_checks():
    lib = _hip.lib()
    assert lib.sx_cnf_train_lds_bytes(_net(3, [8], act=_hip.ACT_CODES['SiLU']), 1) == 0
    assert lib.sx_cnf_train_lds_bytes(None, 1) == 0
    d = _net(3, [8])
    assert lib.sx_cnf_train_fwd(d, 64, None, 64, 64, 64, None, 4, 7, 1, 0.0, 1.0, 0.0, None) != 0          # solver
    assert lib.sx_cnf_train_fwd(d, 64, None, None, 64, 64, None, 4, 2, 1, 0.0, 1.0, 0.0, None) != 0        # noise
    assert lib.sx_cnf_train_fwd(d, 64, None, 64, 64, 64, None, 0, 2, 1, 0.0, 1.0, 0.0, None) == 0          # no rows: nothing to do


def test_module_plan_at_the_coverage_edges():
    cpu = torch.device('cpu')
    assert th.make(3, [5])._train_kernel_net(0, cpu) is not None
    assert th.make(5, [32, 32], latent=58)._train_kernel_net(58, cpu) is not None
    assert th.make(3, [65])._train_kernel_net(0, cpu) is None
    assert th.make(33, [8])._train_kernel_net(0, cpu) is None
    assert th.make(5, [8], latent=59)._train_kernel_net(59, cpu) is None                # 1 + dim + latent = 65
    assert th.make(3, [8, 8, 8])._train_kernel_net(0, cpu) is None
    assert th.make(3, [8], net_kw={'final_activation': 'Tanh'})._train_kernel_net(0, cpu) is None
    assert th.make(3, [8], activation='SiLU')._train_kernel_net(0, cpu) is None
    assert th.make(3, [8], activation=torch.nn.ELU(alpha=2.0))._train_kernel_net(0, cpu) is None


@pytest.mark.parametrize('latent', [0, 3])
@pytest.mark.parametrize('act', th.ACTIVATIONS)
@pytest.mark.parametrize('hidden', [[7], [7, 5]])
def test_restatement_agrees_with_reverse_mode_twice(hidden, act, latent):
    torch.manual_seed(sum(map(ord, act)) + len(hidden) + latent)
    dim, n = 4, 6
    f = th.make(dim, hidden, latent=latent, activation=act).double()
    lins = th.linears(f)
    ws, bs = [l.weight for l in lins], [l.bias for l in lins]
    z = torch.randn(n, dim, dtype=torch.float64, requires_grad=True)
    lat = torch.randn(n, latent, dtype=torch.float64, requires_grad=True) if latent else None
    e = torch.randn(n, dim, dtype=torch.float64)
    kb, qb = torch.randn(n, dim, dtype=torch.float64), torch.randn(n, dtype=torch.float64)
    t = 0.37
    k, q, g = cnf.hutchinson_closed_form(ws, bs, act, t, z, e, lat, kb, qb)
    dv = f.odefunc.diffeq(torch.tensor([t], dtype=torch.float64), z, latent=lat)
    div = (torch.autograd.grad(dv, z, e, create_graph=True)[0] * e).sum(-1)
    wrt = [z] + ([lat] if latent else []) + [p for l in lins for p in (l.weight, l.bias)]
    want = torch.autograd.grad((dv * kb).sum() + (div * qb).sum(), wrt, allow_unused=True)
    want = [torch.zeros_like(w) if a is None else a for a, w in zip(want, wrt)]
    got = [g['z']] + ([g['latent']] if latent else []) + [p for pair in zip(g['W'], g['b']) for p in pair]

    def close(a, b, what):
        assert a.shape == b.shape, what
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), (what, (a - b).abs().max().item())
    close(k, dv, 'k')
    close(q, div, 'q')
    for i, (a, b) in enumerate(zip(got, want)):
        close(a, b, i)
    k2, q2 = cnf.hutchinson_closed_form(ws, bs, act, t, z, e, lat)
    assert torch.equal(k2, k) and torch.equal(q2, q)
