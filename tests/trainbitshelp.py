"""The cases of tests/golden/f25_train_parent_bits.npz, shared by tools/make_train_parent_bits.py (which records what the library it
is run against produces) and tests/test_gpu_train_parent_bits.py (which holds later builds to those bits): the three one-launch
training backward kernels -- sx_resnet_flow_bwd, sx_equivariant_bwd, sx_cnf_train_bwd -- at the smallest shapes that reach each piece
of their shared weight-gradient contraction (stribor_amd/csrc/sx_train_contract.h), and one multi-pass batch per kernel.

A case is a function -> {name: tensor}: every parameter gradient whole, row outputs cut to their first 257 rows.  The nets and
batches are those of the kernels' own test modules (imported, not restated).  MULTI cases run more than SX_*_MAX_BLOCKS = 512
workgroups' worth of rows or sets, so every wave adds to its partial in place (first == false) and the ordered sum walks every slot;
their grid is min(512, CUs x resident workgroups), hence a function of the device: only their parameter gradients are stored, and
the fixture's meta names the CU count it was written on."""
import copy

import torch

import cnftrainhelp as cth
import passhelp as ph
import test_gpu_equivariant as teq
import test_gpu_iresnet_train as tir

DEV = 'cuda'
ROWS = 129                 # five row groups, the last partial, over two workgroups
HEAD = 257
MAX_BLOCKS = 512           # SX_RESNET_BWD_MAX_BLOCKS, SX_EQ_BWD_MAX_BLOCKS, SX_CNF_TRAIN_MAX_BLOCKS
BIG_ROWS = 128 * (2 * MAX_BLOCKS + 1) + 45        # two full trips of the largest grid, one workgroup more, a ragged tail
BIG_SETS_33 = 3 * (2 * MAX_BLOCKS + 1) + 2        # sets of 33: three per pass


def _named(prefix, tensors):
    return {f'{prefix}{i}': t for i, t in enumerate(tensors)}


# ---- sx_resnet_flow_bwd ---------------------------------------------------------------------------------------------------------------
def _resnet(name, inverse, rows=ROWS, params_only=False):
    f, cont, seed = tir.build(name, False)
    x, t, cot = tir.batch(f, cont, seed, rows, key=(name, inverse))
    y, gx, gt, gp = tir.run(f, x, t, cot, inverse=inverse)
    assert f._last_grad_path == 'kernel', name
    out = _named('param', gp)
    if not params_only:
        out.update(y=y[:HEAD], gx=gx[:HEAD])
        if gt is not None:
            out['gt'] = gt[:HEAD]
    return out


# ---- sx_equivariant_bwd ---------------------------------------------------------------------------------------------------------------
def _sets(net, x, mask, gy, params_only=False):
    dev = copy.deepcopy(net).to(DEV)
    y, grads, path = teq._gpu(dev, x.to(DEV), None if mask is None else mask.to(DEV), gy.to(DEV))
    assert path == 'kernel'
    out = _named('param', grads[1:])
    if not params_only:
        out.update(y=y.reshape(-1, y.shape[-1])[:HEAD], dx=grads[0].reshape(-1, x.shape[-1])[:HEAD])
    return out


def _ten_sets(masked):
    net, x, gy = teq._ten_sets()
    mask = (torch.rand(10, 33, 1, generator=ph.generator('det-mask')) < 0.8).float() if masked else None
    return _sets(net, x, mask, gy)


def _set_edge(name):
    (B, N, D, hidden, out), act, fact, path = teq.EDGES[name]
    assert path == 'kernel'
    net = teq._net(11, D, hidden, out, activation=act, final_activation=fact)
    x = torch.randn(B, N, D, generator=ph.generator(name))
    return _sets(net, x, None, torch.randn(B, N, out, generator=torch.Generator().manual_seed(0)))


def _sets_multi():
    net = teq._net(16, 4, [8], 3)
    g = ph.generator('train-bits-sets')
    xs, gs = torch.randn(ph.SET_PERIOD, 33, 4, generator=g), torch.randn(ph.SET_PERIOD, 33, 3, generator=g)
    return _sets(net, ph.tile(xs, BIG_SETS_33), None, ph.tile(gs, BIG_SETS_33), params_only=True)


# ---- sx_cnf_train_fwd / sx_cnf_train_bwd ------------------------------------------------------------------------------------------------
def _cnf(hidden, solver, rows=ROWS, latent=5, params_only=False, step=0.25):
    f = cth.make(3, hidden, latent=latent, solver=solver, step=step, seed=len(hidden)).to(DEV)
    g = ph.generator(f'train-bits-cnf-{len(hidden)}-{solver}')
    x = ph.tile(torch.randn(min(rows, ph.ROW_PERIOD * 2), 3, generator=g), rows).to(DEV)
    lat = ph.tile(torch.randn(min(rows, ph.ROW_PERIOD * 2), latent, generator=g), rows).to(DEV)
    got = cth.run(f, x, lat)
    assert got['path'] == 'kernel'
    out = _named('param', got['params'])
    if not params_only:
        out.update(y=got['y'][:HEAD], ldj=got['ldj'][:HEAD], gx=got['gx'][:HEAD], g_latent=got['glat'][:HEAD])
    return out


CASES = {
    'resnet/d8_relu_tanh/forward': lambda: _resnet('d8_relu_tanh', False),              # one tile each way
    'resnet/d8_relu_tanh/inverse': lambda: _resnet('d8_relu_tanh', True),
    'resnet/d64_silu_log/forward': lambda: _resnet('d64_silu_log', False),              # two tiles each way
    'resnet/d64_silu_log/inverse': lambda: _resnet('d64_silu_log', True),
    'resnet/d3_empty/forward': lambda: _resnet('d3_empty', False),                      # no hidden layer: NL == 1
    'resnet/d3_empty/inverse': lambda: _resnet('d3_empty', True),
    'sets/ten_sets': lambda: _ten_sets(False),                                          # N = 33: sets straddle waves, padding slots
    'sets/ten_sets_masked': lambda: _ten_sets(True),
    'sets/bwd_edge_inside': lambda: _set_edge('bwd_edge_inside'),                       # three layers, two output tiles
    'sets/bwd_edge_inside_one_hidden_64': lambda: _set_edge('bwd_edge_inside_one_hidden_64'),       # two hidden tiles
    'cnf/h1/euler': lambda: _cnf([16], 'euler'),
    'cnf/h1/rk4': lambda: _cnf([16], 'rk4'),
    'cnf/h2/euler': lambda: _cnf([16, 12], 'euler'),
    'cnf/h2/rk4': lambda: _cnf([16, 12], 'rk4'),
}
MULTI = {
    'multi/resnet/d4_iresnet': lambda: _resnet('d4_iresnet', False, rows=BIG_ROWS, params_only=True),
    'multi/sets/n33': _sets_multi,
    'multi/cnf/h1/euler': lambda: _cnf([8], 'euler', rows=BIG_ROWS, latent=2, params_only=True, step=0.35),
}


def run(name):
    """One case -> {array name: fp32 CPU tensor}."""
    torch.manual_seed(0)
    return {k: v.detach().float().cpu().contiguous() for k, v in {**CASES, **MULTI}[name]().items()}


def same_bits(a, b):
    """torch.equal, with NaNs matching NaNs."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def cu_count():
    return torch.cuda.get_device_properties(DEV).multi_processor_count
