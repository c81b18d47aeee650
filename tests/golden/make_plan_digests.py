#!/usr/bin/env python3
"""Digest what the host-side planner (stribor_amd/fused.py, ProgramBuilder) produces for a corpus of flows.

Unlike the other make_golden*.py scripts this one reads nothing but this project: the fixture pins the planner against ITSELF, so
that a change meant to leave every plan as it is (a refactor of ProgramBuilder) can be proved byte for byte on the CPU.

    python tests/golden/make_plan_digests.py          # writes tests/golden/plan_digests.json

Run it on the commit whose plans are the reference (an unmodified checkout), never to make a failing test pass.  The module is
also the corpus of tests/test_plan_digest.py, which imports CASES / REFUSALS / record().

Per case the fixture holds {"kinds": [...], "digest": sha256} or the string "raises" (the planner refused with
NotImplementedError) or null (the flow-level builder returned None / 'unsupported': the flow keeps another tier).  "kinds" is the
step-kind sequence of every program of the case, run-length coded ("11*12" = twelve steps of kind 11), in clear so that a
mismatch says where the plan diverged.  The digest covers, per program: the whole sx_program struct, blob_floats, the column
maps, mlp_out_dim / mlp_col0 / accumulates, and of every job its class name and every host-side field (index arrays with dtype
and shape, scales, gathers, pad tables, scalars, tile counts, offsets, flags; of tensors only the shape / None-ness).
"""
import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flowdesc as fd  # noqa: E402
import stribor_amd as st  # noqa: E402
from stribor_amd import _hip  # noqa: E402
from stribor_amd.fused import CompiledProgram, ProgramBuilder  # noqa: E402
from stribor_amd.net.mlp import BatchLinear  # noqa: E402

FIXTURE = os.path.join(HERE, 'plan_digests.json')
CPU = torch.device('cpu')
TANH, RELU = _hip.ACT_CODES['Tanh'], _hip.ACT_CODES['ReLU']


# ---- digest ------------------------------------------------------------------------------------------------------------
def _feed(h, tag, v):
    """One field into the hash: values of host data, shapes only of tensors, nothing of pointers / ids / callables."""
    h.update(tag.encode() + b'=')
    if v is None:
        h.update(b'none;')
    elif isinstance(v, np.generic):
        _feed(h, '', v.item())
    elif isinstance(v, (bool, int)):
        h.update(b'i%d;' % int(v))
    elif isinstance(v, float):
        h.update(b'f' + v.hex().encode() + b';')
    elif isinstance(v, str):
        h.update(b's' + v.encode() + b';')
    elif isinstance(v, np.ndarray):
        h.update(f'a{v.dtype.str}{v.shape}'.encode())
        h.update(np.ascontiguousarray(v).tobytes() + b';')
    elif torch.is_tensor(v):
        h.update(f't{tuple(v.shape)};'.encode())
    elif isinstance(v, (list, tuple)):
        h.update(b'[%d' % len(v))
        for i, x in enumerate(v):
            _feed(h, str(i), x)
        h.update(b'];')
    elif isinstance(v, dict):
        h.update(b'{')
        for k in sorted(v):
            _feed(h, str(k), v[k])
        h.update(b'};')
    elif isinstance(v, torch.nn.Module):
        h.update(b'm' + type(v).__name__.encode() + b';')
    elif callable(v):
        h.update(b'fn;')
    else:
        raise TypeError(f'plan digest: field {tag!r} holds a {type(v).__name__}')


def _feed_jobs(h, jobs):
    h.update(b'jobs%d;' % len(jobs))
    for j in jobs:
        h.update(type(j).__name__.encode() + b':')
        for k in sorted(vars(j)):
            _feed(h, k, getattr(j, k))


def _step_bytes(s) -> bytes:
    """A builder's step dict as the sx_step it becomes (what ProgramBuilder.build does with it)."""
    stp = _hip.sx_step()
    for k, v in s.items():
        setattr(stp, k, v)
    return bytes(stp)


def _rle(kinds):
    out = []
    for k in kinds:
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return ' '.join(str(k) if n == 1 else f'{k}*{n}' for k, n in out)


def _feed_plan(h, kinds, obj):
    if isinstance(obj, CompiledProgram):
        kinds.append(_rle(obj.prog.steps[i].kind for i in range(obj.prog.n_steps)))
        h.update(b'program:' + bytes(obj.prog))
        for k in ('blob_floats', 'mlp_out_dim', 'mlp_col0', 'accumulates'):
            _feed(h, k, getattr(obj, k))
        for k in ('in_col', 'out_col'):
            t = getattr(obj, k)
            _feed(h, k, None if t is None else t.numpy())
        _feed(h, 'owned', obj._owner is not None)
        _feed_jobs(h, obj.jobs)
    elif isinstance(obj, ProgramBuilder):
        kinds.append(_rle(s['kind'] for s in obj.steps))
        h.update(b'builder:')
        for s in obj.steps:
            h.update(_step_bytes(s))
        for k in ('blob_floats', 'mlp_out_dim', 'tiles', 'x_tiles', 'h_tiles', 'col_of_slot', 'in_col'):
            _feed(h, k, getattr(obj, k))
        _feed_jobs(h, obj.jobs)
    elif isinstance(obj, (list, tuple)):
        h.update(b'(%d' % len(obj))
        for x in obj:
            _feed_plan(h, kinds, x)
        h.update(b')')
    else:
        _feed(h, 'value', obj)          # e.g. the slot maps add_coupling_affine_bwd returns


def record(thunk):
    """The fixture entry of one case: 'raises' | None | {'kinds': [...], 'digest': hex}."""
    torch.manual_seed(0)
    try:
        got = thunk()
    except NotImplementedError:
        return 'raises'
    if got is None or isinstance(got, str):          # _build_fused: None; _build_backward_program: 'unsupported'
        return None
    h, kinds = hashlib.sha256(), []
    _feed_plan(h, kinds, got)
    return {'kinds': kinds, 'digest': h.hexdigest()}


# ---- corpus ------------------------------------------------------------------------------------------------------------
CASES = {}          # name -> thunk (run under torch.manual_seed(0))
REFUSALS = set()    # the cases whose entry is 'raises' or null: the only ones a digest is not compared for


def case(name, thunk, refusal=False):
    assert name not in CASES, name
    CASES[name] = thunk
    if refusal:
        REFUSALS.add(name)


def flow_cases(name, make, dim, latent_dim=0, t_kind=None, refusal=()):
    """A whole flow through NormalizingFlow._build_fused, one case per direction; make() -> list of transforms | desc list."""
    def run(reverse):
        parts = make()
        ts = [fd.build_transform(st, d) if isinstance(d, dict) else d for d in parts]
        return st.NormalizingFlow(st.UnitNormal(dim), ts)._build_fused(reverse, dim, latent_dim, CPU, t_kind)
    for tag, reverse in (('fwd', False), ('inv', True)):
        case(f'{name}/{tag}', lambda reverse=reverse: run(reverse), refusal=refusal is True or tag in refusal)


def affine(dim, hidden, mask, latent_dim=0, act='Tanh'):
    return st.Coupling(st.Affine(dim, latent_net=st.net.MLP(dim + latent_dim, list(hidden), 2 * dim, activation=act)), mask=mask)


def rqs(dim, hidden, mask, K, latent_dim=0, cubic=False):
    return {'kind': 'coupling_rqs', 'dim': dim, 'hidden': list(hidden), 'n_bins': K, 'lower': -3, 'upper': 3, 'mask': mask,
            'latent_dim': latent_dim, 'spline_type': 'cubic' if cubic else 'quadratic'}


def halves(n, make):
    return [make('ordered_right_half' if i % 2 == 0 else 'ordered_left_half') for i in range(n)]


def lin(i, o):
    m = torch.nn.Linear(i, o)
    return m.weight, m.bias


def split_mask(dim, low_cond=False):
    m = np.zeros(dim)
    m[:dim // 2] = 1 if low_cond else 0
    m[dim // 2:] = 0 if low_cond else 1
    return m


# baseline configs at their own dims
flow_cases('cfg1', lambda: [{'kind': 'affine', 'dim': 2}], 2)
flow_cases('cfg2', fd.cfg2_desc, 64)
flow_cases('cfg3', fd.cfg3_desc, 64)
flow_cases('cfg4', fd.cfg4_desc, 128)

# affine couplings: masks
flow_cases('affine/halves', lambda: fd.cfg2_desc(2), 64)                                   # pruned high, then low
flow_cases('affine/halves128', lambda: fd.cfg2_desc(2, dim=128, hidden=64), 128)
flow_cases('affine/halves48', lambda: halves(2, lambda m: affine(48, [40], m)), 48)       # re-laid out: 24 + 24 in two tiles
flow_cases('affine/parity', lambda: [affine(64, [64], 'parity_even'), affine(64, [64], 'parity_odd')], 64)
flow_cases('affine/halves_then_parity', lambda: [affine(64, [64], 'ordered_right_half'), affine(64, [64], 'parity_even')], 64)
flow_cases('affine/permute_dense', lambda: [affine(64, [64], 'ordered_right_half'), st.Permute(64),
                                            affine(64, [64], 'ordered_left_half')], 64)
flow_cases('affine/parity_permute_flip', lambda: [affine(40, [32], 'parity_even'), st.Permute(40), affine(40, [32], 'parity_odd'),
                                                  st.Flip([-1]), affine(40, [32], 'ordered_left_half')], 40)
flow_cases('affine/dim1', lambda: [affine(1, [16], 'ordered_right_half')], 1)
flow_cases('affine/dim1_deep', lambda: [affine(1, [16, 12], 'ordered_right_half')], 1)
flow_cases('affine/dim20', lambda: halves(2, lambda m: affine(20, [24], m)), 20)          # one tile: dense
flow_cases('affine/mask_none', lambda: [affine(8, [16], 'none')], 8)
flow_cases('affine/latent3', lambda: halves(2, lambda m: affine(20, [32], m, latent_dim=3)), 20, latent_dim=3)
flow_cases('affine/latent3_dim40', lambda: halves(2, lambda m: affine(40, [32], m, latent_dim=3)), 40, latent_dim=3)    # 2 data + 1 latent tile of 4
flow_cases('affine/hidden300', lambda: halves(2, lambda m: affine(64, [300], m)), 64)     # COUPLING_AFFINE_HC, three chunks
flow_cases('affine/hidden300_dim128', lambda: halves(2, lambda m: affine(128, [300], m)), 128)     # chunks of 64 units
flow_cases('affine/wide200', lambda: halves(2, lambda m: affine(200, [64], m)), 200)     # WIDE_HIDDEN / WIDE_AFFINE_TILE
flow_cases('affine/wide180', lambda: halves(2, lambda m: affine(180, [64], m)) + [st.Affine(180)], 180)   # + a padding-only tile
flow_cases('affine/relu', lambda: halves(2, lambda m: affine(64, [64], m, act='ReLU')), 64)       # unfolded scales
flow_cases('affine/elu_dense', lambda: [affine(24, [20], 'parity_even', act='ELU')], 24)
flow_cases('affine/deep2', lambda: halves(2, lambda m: affine(64, [48, 40], m)), 64)
flow_cases('affine/deep3', lambda: halves(2, lambda m: affine(64, [48, 40, 36], m)), 64)
flow_cases('affine/deep2_latent_relu', lambda: [affine(20, [48, 40], 'parity_odd', latent_dim=3, act='ReLU')], 20, latent_dim=3)


def _scalar_mask():
    b = ProgramBuilder(8, 0, 16)
    for reverse, m in ((False, np.array([0.0])), (True, np.array(1.0))):       # mask.py 'none' is zeros(1); a 0-dim 1 as well
        b.add_coupling_affine(*lin(8, 16), *lin(16, 16), m, TANH, reverse, 1.0, 16)
        b.add_coupling_affine_deep([lin(8, 16), lin(16, 12), lin(12, 16)], m, TANH, reverse, 1.0)
        b.add_coupling_rqs(*lin(8, 16), *lin(16, 8 * 11), m, reverse, 1.0, 16, 4, -1.0, 1.0, -2.0, 2.0)
    return b


case('affine/scalar_mask_direct', _scalar_mask)

# spline couplings
for K in (4, 16, 20):
    for hidden in ([64], [48, 40], [48, 40, 36]):
        flow_cases(f'rqs/K{K}_h{len(hidden)}', lambda K=K, hidden=hidden: halves(2, lambda m: rqs(64, hidden, m, K)), 64)
flow_cases('rqs/cubic8', lambda: halves(2, lambda m: rqs(64, [64], m, 8, cubic=True)), 64)
flow_cases('rqs/cubic16_deep', lambda: halves(2, lambda m: rqs(64, [48, 40], m, 16, cubic=True)), 64)
flow_cases('rqs/dim40', lambda: halves(2, lambda m: rqs(40, [32], m, 5)), 40)              # dead slots and dead groups
flow_cases('rqs/dim34_K20', lambda: [rqs(34, [32], 'ordered_right_half', 20)], 34)    # a group with one live element pair
flow_cases('rqs/dim40_K20', lambda: [rqs(40, [32], 'parity_even', 20)], 40)
flow_cases('rqs/latent3', lambda: halves(2, lambda m: rqs(20, [32], m, 6, latent_dim=3)), 20, latent_dim=3)
flow_cases('rqs/latent3_deep', lambda: [rqs(20, [32, 24], 'parity_even', 6, latent_dim=3)], 20, latent_dim=3)
flow_cases('rqs/dim1', lambda: [rqs(1, [16], 'ordered_right_half', 4)], 1)
flow_cases('mixed/rqs_affine_sigmoid', lambda: [rqs(64, [64], 'ordered_right_half', 16), fd.cfg2_desc(1)[0], st.Sigmoid()], 64)
flow_cases('mixed/cubic_quadratic_deep', lambda: [rqs(64, [64], 'ordered_right_half', 16, cubic=True),
                                                  rqs(64, [64], 'ordered_left_half', 16), affine(64, [48, 40], 'ordered_left_half')], 64)
flow_cases('rqs/too_long', lambda: fd.cfg3_desc(16), 64, refusal=True)                     # 208 steps: ProgramTooLong -> None


def _segments():
    flow = fd.build_flow(st, fd.cfg3_desc(16), 64)
    assert flow._build_fused(True, 64, 0, CPU) is None
    return flow._fused_segments(True, 64, 0, CPU)           # snapshot / restore of the builder between layers


case('rqs/segments', _segments)


# time-conditioned couplings, through NeuralFlow._fused (with_t0: the inverse pass at t0, then the forward pass at t)
def time_flow(kind, cat, dim=6, latent_dim=0, with_t0=True, masks=('ordered_right_half', 'ordered_left_half'), **kw):
    def run():
        ts = [fd.build_transform(st, dict({'kind': 'continuous_affine_coupling', 'dim': dim, 'hidden': [24], 'mask': m,
                                           'latent_dim': latent_dim, 'time_kind': kind, 'concatenate_time': cat}, **kw)) for m in masks]
        return st.NeuralFlow(ts)._fused(dim, latent_dim, with_t0, CPU)
    return run


for kind in ('identity', 'linear', 'tanh', 'log', 'fourier', 'fourier_bounded'):
    for cat in (True, False):
        case(f'time/{kind}_{"cat" if cat else "nocat"}', time_flow(kind, cat))
case('time/tanh_no_t0', time_flow('tanh', True, with_t0=False))
case('time/linear_latent3', time_flow('linear', True, latent_dim=3))
case('time/fourier_latent40_dim40', time_flow('fourier', True, dim=40, latent_dim=40, time_hidden=3))      # 2 data + 2 latent tiles
case('time/tanh_broadcast', time_flow('tanh', False, time_out=2))
case('time/log_dim1', time_flow('log', True, dim=1))
case('time/identity_dim90_parity', time_flow('identity', True, dim=90, masks=('parity_even', 'parity_odd')))   # 3 data tiles + the time tile


def _time_relu():
    b = ProgramBuilder(6, 0, 24, time_slots=1)
    b.add_coupling_time(*lin(7, 24), *lin(24, 12), np.array([1.0, 1, 1, 0, 0, 0]), RELU, True, -1.0, 24, 6, 0, st.net.TimeTanh(12))
    return b


case('time/relu_direct', _time_relu)


# backward programs of log_prob
def bwd(make, dim):
    def run():
        ts = [fd.build_transform(st, d) if isinstance(d, dict) else d for d in make()]
        got = st.NormalizingFlow(st.UnitNormal(dim), ts)._build_backward_program(dim, CPU)
        if isinstance(got, str):
            return got
        prog, layers = got
        return [prog, [{k: v for k, v in info.items() if k not in ('slot_map', 'row_map', 'col_map')} for _, info in layers]]
    return run


case('bwd/xt1', bwd(lambda: halves(2, lambda m: affine(20, [24], m)), 20))
case('bwd/xt2_halves', bwd(lambda: fd.cfg2_desc(2), 64))
case('bwd/xt2_parity', bwd(lambda: [affine(64, [64], 'parity_even'), affine(64, [64], 'parity_odd')], 64))
case('bwd/xt2_dense', bwd(lambda: [affine(64, [32], 'ordered_right_half'), st.Permute(64), affine(64, [32], 'ordered_left_half')], 64))
case('bwd/xt2_dim40', bwd(lambda: halves(2, lambda m: affine(40, [32], m)), 40))
case('bwd/xt4_halves', bwd(lambda: fd.cfg2_desc(2, dim=128, hidden=64), 128))
case('bwd/xt4_dim100', bwd(lambda: halves(2, lambda m: affine(100, [48], m)) + [st.Affine(100)], 100), refusal=True)   # an Affine: unsupported
case('bwd/xt4_linear', bwd(lambda: fd.cfg4_desc(1), 128))                                  # add_linear_bwd, 4 + 4 tiles
case('bwd/xt4_dense', bwd(lambda: [affine(128, [64], 'ordered_right_half'), st.Permute(128), affine(128, [64], 'ordered_left_half')], 128),
     refusal=True)


def _bwd_direct(dim, hidden, mask, min_x_tiles=1, builder_hidden=None):
    def run():
        b = ProgramBuilder(dim, 0, builder_hidden or hidden, min_x_tiles=min_x_tiles)
        b.enable_adjoint_tiles()
        info = b.add_coupling_affine_bwd(*lin(dim, hidden), *lin(hidden, 2 * dim), mask, hidden, 3)
        return [b, info]
    return run


case('bwd/direct_xt4_dim100', _bwd_direct(100, 48, split_mask(128)[:100], min_x_tiles=4))   # halves of the TILES at 100 columns
case('bwd/direct_scalar_mask', _bwd_direct(20, 24, np.array([0.0])))
case('bwd/direct_dim1', _bwd_direct(1, 8, np.ones(1)))

# other steps
flow_cases('other/affine_const', lambda: [st.Affine(40), affine(40, [32], 'parity_even'), st.Affine(40)], 40)
flow_cases('other/pointwise', lambda: [st.Sigmoid(), affine(40, [32], 'ordered_right_half'), st.Logit(), st.ELU(), st.LeakyReLU(0.2)], 40)
flow_cases('other/affine_lu', lambda: [st.AffineLU(40), affine(40, [32], 'parity_even'), st.AffineLU(40)], 40)
flow_cases('other/matrix_exp', lambda: [st.MatrixExponential(40, bias=True), affine(40, [32], 'parity_even')], 40)
flow_cases('other/matrix_exp_time', lambda: [st.MatrixExponential(40, bias=True, log_time=True), affine(40, [32], 'parity_even'),
                                             st.MatrixExponential(40)], 40, t_kind='tensor')
flow_cases('other/affine_only_wide', lambda: [st.Affine(200)], 200, refusal=True)           # eight tiles without a coupling


# MLP programs
def mlp(in_dim, hidden, out_dim, act='Tanh'):
    return lambda: st.net.MLP(in_dim, hidden, out_dim, activation=act)._program(CPU)


case('mlp/one_hidden', mlp(20, [48], 77))
case('mlp/two_hidden', mlp(20, [48, 40], 77, act='ReLU'))
case('mlp/three_hidden', mlp(100, [128, 33, 64], 32))
case('mlp/hidden300', mlp(20, [300], 50))                                                  # hidden_rows + accumulate
case('mlp/511_tiles', mlp(20, [48], 8192 + 2 * 4032 + 77))


def conditioner(dim, hidden, latent_dim, mask, spline=None):
    def run():
        c = fd.build_transform(st, rqs(dim, hidden, mask, spline, latent_dim)) if spline else affine(dim, hidden, mask, latent_dim)
        m = c.mask_vector(dim)
        live = np.nonzero(m <= 0.5)[0]
        P = c.transform.params_per_element if spline else 0
        out_rows = (live[:, None] * P + np.arange(P)[None, :]).reshape(-1) if spline else np.concatenate([live, dim + live])
        return c._conditioner_programs(dim, latent_dim, CPU, m > 0.5, out_rows)
    return run


case('mlp/conditioner', conditioner(64, [64], 0, 'parity_even'))                           # in_cols_live
case('mlp/conditioner_latent', conditioner(20, [32, 24], 3, 'ordered_left_half'))
case('mlp/conditioner_wide', conditioner(200, [300], 0, 'ordered_right_half'))             # w1_cols + hidden_rows + accumulate
case('mlp/conditioner_wide_latent', conditioner(150, [64], 3, 'parity_odd'))               # ... + w1_latent_base
case('mlp/conditioner_spline', conditioner(40, [32], 0, 'ordered_right_half', spline=6))
case('mlp/conditioner_too_wide', conditioner(300, [300], 0, 'ordered_right_half'), refusal=True)
case('mlp/time_conditioner', lambda: fd.build_transform(st, {
    'kind': 'continuous_affine_coupling', 'dim': 6, 'hidden': [24], 'mask': 'parity_even', 'latent_dim': 2, 'time_kind': 'tanh'})
     ._program(6, 3, CPU)[0])


def single_linear(i, o, transpose):
    def run():
        W, b = lin(i, o)
        return BatchLinear._linear_programs(W.detach(), None if transpose else b.detach(), transpose, CPU)
    return run


case('linear/plain', single_linear(100, 70, False))
case('linear/plain_k0', single_linear(300, 40, False))                                     # three programs, k0 = 0 / 128 / 256
case('linear/transpose_k0', single_linear(64, 200, True))                                  # W^T, two programs, the second at k0 = 128


# refusals: NotImplementedError out of the builder itself
def _raises_in_ctor():
    return ProgramBuilder(300, 0, 32)


def direct(dim, hidden, call, **kw):
    def run():
        b = ProgramBuilder(dim, 0, hidden, **kw)
        call(b)
        return b
    return run


m64 = split_mask(64, True)
m200 = (np.arange(200) >= 128).astype(np.float64)          # splits the eight tiles' halves in the identity layout
parity64 = (np.arange(64) % 2).astype(np.float64)
case('refuse/dim300', _raises_in_ctor, refusal=True)
case('refuse/hc_relu', direct(64, 300, lambda b: b.add_coupling_affine(*lin(64, 300), *lin(300, 128), m64, RELU, True, -1.0, 300)), refusal=True)
case('refuse/hc_dense', direct(64, 300, lambda b: b.add_coupling_affine(*lin(64, 300), *lin(300, 128), parity64, TANH, True, -1.0, 300)),
     refusal=True)
case('refuse/rqs_hidden300', direct(64, 300, lambda b: b.add_coupling_rqs(*lin(64, 300), *lin(300, 128), m64, True, -1.0, 300, 4, -1, 1, -1, 1)),
     refusal=True)
case('refuse/mlp_deep_150', direct(64, 150, lambda b: b.add_mlp([lin(64, 150), lin(150, 69), lin(69, 94)], TANH, None, np.arange(94))),
     refusal=True)


def _bwd_hidden150():
    b = ProgramBuilder(64, 0, 150, min_x_tiles=1)
    b.enable_adjoint_tiles()
    b.add_coupling_affine_bwd(*lin(64, 150), lin(150, 128)[0], torch.zeros(128), m64, 150, 0)


case('refuse/bwd_hidden150', _bwd_hidden150, refusal=True)
case('refuse/wide_relu', direct(200, 64, lambda b: b.add_coupling_affine(*lin(200, 64), *lin(64, 400), m200, RELU, False, 1.0, 64)), refusal=True)
case('refuse/wide_dense', direct(200, 64, lambda b: b.add_coupling_affine(*lin(200, 64), *lin(64, 400), (np.arange(200) % 2).astype(float),
                                                                          TANH, False, 1.0, 64)), refusal=True)
case('refuse/wide_hidden300', direct(200, 300, lambda b: b.add_coupling_affine(*lin(200, 300), *lin(300, 400), m200, TANH, False, 1.0, 300)),
     refusal=True)
case('refuse/wide_deep', direct(200, 64, lambda b: b.add_coupling_affine_deep([lin(200, 64), lin(64, 48), lin(48, 400)], m200, TANH, False, 1.0)),
     refusal=True)
case('refuse/deep_hidden150', direct(64, 150, lambda b: b.add_coupling_affine_deep([lin(64, 150), lin(150, 48), lin(48, 128)], m64, TANH, False, 1.0)),
     refusal=True)
case('refuse/rqs_K33', direct(64, 64, lambda b: b.add_coupling_rqs(*lin(64, 64), *lin(64, 64 * 98), m64, False, 1.0, 64, 33, -3, 3, -3, 3)),
     refusal=True)
case('refuse/cubic_K17', direct(64, 64, lambda b: b.add_coupling_rqs(*lin(64, 64), *lin(64, 64 * 36), m64, False, 1.0, 64, 17, -3, 3, -3, 3,
                                                                     cubic=True)), refusal=True)
case('refuse/bwd_xt4_dense', _bwd_direct(128, 64, (np.arange(128) % 2).astype(float)), refusal=True)
case('refuse/bwd_latent', lambda: ProgramBuilder(20, 3, 32).enable_adjoint_tiles(), refusal=True)
case('refuse/bwd_xt4_hidden128', lambda: ProgramBuilder(128, 0, 128).enable_adjoint_tiles(), refusal=True)


def _linear_bwd_narrow():
    b = ProgramBuilder(40, 0, 32)
    b.enable_adjoint_tiles()
    b.add_linear_bwd([], None, None, 0)


case('refuse/linear_bwd_narrow', _linear_bwd_narrow, refusal=True)
case('refuse/time_fourier65', direct(6, 24, lambda b: b.add_coupling_time(*lin(7, 24), *lin(24, 12), np.ones(6), TANH, False, 0.0, 24, 6, 0,
                                                                          st.net.TimeFourier(12, 65)), time_slots=1), refusal=True)
case('refuse/lds_limit', direct(128, 128, lambda b: b.add_coupling_affine(*lin(128, 128), *lin(128, 256), (np.arange(128) % 2).astype(float),
                                                                          TANH, False, 1.0, 128)), refusal=True)
case('refuse/time_hidden200', direct(6, 200, lambda b: b.add_coupling_time(*lin(7, 200), *lin(200, 12), np.ones(6), TANH, False, 0.0, 200, 6, 0,
                                                                           st.net.TimeTanh(12)), time_slots=1), refusal=True)
case('refuse/time_no_slot', direct(6, 24, lambda b: b.add_coupling_time(*lin(7, 24), *lin(24, 12), np.ones(6), TANH, False, 0.0, 24, 6, 1,
                                                                        st.net.TimeTanh(12)), time_slots=1), refusal=True)
case('refuse/pointwise_wide', direct(200, 64, lambda b: b.add_pointwise(1, 0.0, 0.0, 1.0)), refusal=True)
flow_cases('refuse/flow_cubic_K20', lambda: [rqs(64, [64], 'ordered_left_half', 20, cubic=True)], 64, refusal=True)
flow_cases('refuse/flow_rqs_affine_lu', lambda: [rqs(64, [64], 'ordered_right_half', 16), st.AffineLU(64)], 64, refusal=True)
flow_cases('refuse/flow_rqs_cumsum', lambda: [rqs(64, [64], 'ordered_right_half', 16), st.Cumsum(-1)], 64, refusal=True)
flow_cases('refuse/flow_lds_limit', lambda: [affine(128, [128], 'parity_even')], 128, refusal=True)
flow_cases('refuse/flow_wide_deep', lambda: halves(2, lambda m: affine(200, [48, 40], m)), 200, refusal=True)
flow_cases('refuse/flow_hc_with_rqs', lambda: [affine(64, [300], 'ordered_right_half'), rqs(64, [64], 'ordered_left_half', 8)], 64, refusal=True)


def main():
    out, wrong = {}, []
    for name, thunk in CASES.items():
        rec = out[name] = record(thunk)
        if (rec is None or rec == 'raises') != (name in REFUSALS):
            wrong.append(f'{name}: {rec}')
    assert not wrong, 'planned / refused against what the corpus says:\n' + '\n'.join(wrong)
    with open(FIXTURE, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f'{len(out)} cases ({len(REFUSALS)} refusals) -> {FIXTURE}, {os.path.getsize(FIXTURE)} bytes')


if __name__ == '__main__':
    main()
