"""GPU: bf16 storage to the precision of a bf16 store, every stream launcher's dispatch table against fp64, and inputs whose base
pointer is not 16-byte aligned.

Tolerances are measured, not chosen (storagehelp): an fp32 output stays within cnfhelp.bound(ref32, truth64) of the fp64 value -- 8 x
the CPU oracle's own fp32 error, floored at 1e-6 * max(1, max |truth|) --, a bf16 output within half a bf16 ulp of the fp64 value plus
that bound, element by element; pass-through columns, permutations and exact rounding ties are compared bit for bit.  The fp32
reference sequence and the fp64 truth are oracle/stribor_oracle.py on the CPU, fed the values the kernel was given.

The dispatch tables name the kernel each row is meant to reach.  The library does not report the branch it took, so every table is
checked against a restatement of the launcher's own condition (file:line beside it): a table that drifts from the launcher fails."""
import os
import sys

import pytest
import torch

import cnfhelp as ch
import flowdesc as fd
from storagehelp import WORST, Pool, assert_f32, assert_store, bits, offset_view

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import stribor_oracle as orc

import stribor_amd as st
from stribor_amd import _hip

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROWS = (1, 63, 257, 100)          # one row, a partial wave, several workgroups' worth, and a count that leaves a ragged last wave
LDJ = (('none', 1.0), ('over', 1.0), ('over', -1.0), ('acc', 1.0), ('acc', -1.0))     # ldj absent / overwritten / accumulated x ldj_scale


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def gen(seed):
    return torch.Generator().manual_seed(seed)


def put(t, k=0):
    """t on the device; k != 0: with its base pointer k elements past a 16-byte boundary."""
    t = t.to(DEV)
    return offset_view(t, k) if k else t


def stored(x32, bf):
    """(the values the kernel sees as fp32 on the CPU, the tensor in its storage type on the CPU)"""
    if bf:
        xb = x32.bfloat16()
        return xb.float(), xb
    return x32, x32


def pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def ldj_buffer(mode, n, g, k=0):
    """-> (what the buffer holds before the call on the CPU, the device buffer): NaN when the kernel must overwrite without reading."""
    if mode == 'none':
        return None, None
    base = torch.full((n,), float('nan')) if mode == 'over' else torch.randn(n, generator=g) * 3
    return base, put(base, k)


class Case:
    """A dispatch-table case runs at every row count of ROWS.  Its body is walked twice: first without launches, pooling the
    reference's own error per (storage type, direction, output) over the row counts (storagehelp.Pool), then with them, every launch
    held to the case's bound.  Failures are collected, so that one run prints the figures of every launch."""

    def __init__(self, launcher=None):
        self.pool, self.collect, self.launcher, self.refs, self.failed = Pool(), True, launcher, {}, []

    def phases(self):
        for self.collect in (True, False):
            yield self.collect
        assert not self.failed, (len(self.failed), self.failed[:3])

    def cached(self, key, make):
        """reference values: computed in the first walk, reused in the second"""
        if key not in self.refs:
            self.refs[key] = make()
        return self.refs[key]

    def store(self, key, got, ref32, truth64, what, tol=True):
        if self.collect:
            self.pool.add(key, ref32, truth64)
            return
        try:
            assert_store(got, ref32, truth64, what, self.launcher, self.pool.tol(key) if tol else None)
        except AssertionError as e:
            self.failed.append(str(e)[:300])

    def ldj(self, key, mode, scale, got, base, term32, term64, what):
        """ldj = (accumulate ? ldj : 0) + ldj_scale * (the row's log-det term)"""
        if mode == 'none':
            return
        b = base if mode == 'acc' else torch.zeros_like(term32)
        self.store((key, 'ldj', mode, scale), got, b + scale * term32, b.double() + scale * term64, what + ' ldj')

    def columns(self, key, y, x_dev, cols, live32, live64, what):
        """live columns to the storage criterion, every other column bit-identical to the input"""
        if not self.collect:
            check_pass_through(y, x_dev, cols, what)
        self.store((key, 'y'), None if self.collect else y.cpu()[:, cols], live32, live64, what)


def check_pass_through(y, x_dev, cols, what):
    rest = torch.ones(x_dev.shape[1], dtype=torch.bool)
    rest[cols] = False
    assert torch.equal(bits(y)[:, rest], bits(x_dev)[:, rest]), what + ': pass-through columns changed'


def check_ldj(mode, scale, got, base, term32, term64, what, launcher):
    """ldj = (accumulate ? ldj : 0) + ldj_scale * (the row's log-det term), held to this launch's own bound"""
    if mode == 'none':
        return
    b = base if mode == 'acc' else torch.zeros_like(term32)
    assert_f32(got, b + scale * term32, b.double() + scale * term64, what + ' ldj', launcher)


def check_columns(y, x_dev, cols, live32, live64, what, launcher):
    """live columns to the storage criterion (this launch's own bound), every other column bit-identical to the input"""
    check_pass_through(y, x_dev, cols, what)
    assert_store(y.cpu()[:, cols], live32, live64, what, launcher)


# ------------------------------------------------------------------------------------------------------------------------------
# sx_affine_coupling
# ------------------------------------------------------------------------------------------------------------------------------
def affine_call(x, params, pstride, idx, l0, nl, reverse, ldj=None, acc=0, scale=1.0, y=None):
    n, d = x.shape
    y = torch.empty_like(x) if y is None else y
    _hip.call('sx_affine_coupling', x, x.data_ptr(), y.data_ptr(), _hip.ptr(ldj), params.data_ptr(), pstride, _hip.ptr(idx), l0, nl,
              n, d, _hip.dtype_code(x), int(reverse), int(acc), float(scale))
    return y


def affine_vec_expected(x, y, params, pstride, idx, l0, nl):
    """sx_affine_coupling's `fast` condition, restated"""
    d = x.shape[1]
    cpt = 8 if x.dtype == torch.bfloat16 else 4
    return (idx is None and d % cpt == 0 and pow2(d // cpt) and d // cpt <= 64 and l0 % cpt == 0 and nl % cpt == 0 and pstride % 4 == 0
            and l0 + nl <= d and params.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0)


def affine_table(c):
    """(branch, dim, live_start, n_live, params_stride - 2 n_live | 'row', live_idx?, vec kernel?) in units of c = columns per thread
    (fp32 4, bf16 8); the reason a row leaves the vec kernel is the ONE clause of sx_affine_coupling's `fast` condition it violates."""
    return [('vec, dim/cpt = 1', c, 0, c, 0, False, True),
            ('vec, dim/cpt = 2', 2 * c, c, c, 0, False, True),
            ('vec, dim/cpt = 64', 64 * c, 16 * c, 32 * c, 0, False, True),
            ('vec, padded parameter rows (stride % 4 == 0)', 8 * c, 0, 4 * c, 4, False, True),
            ('vec, one broadcast parameter row (stride 0)', 8 * c, 4 * c, 4 * c, 'row', False, True),
            ('generic: dim % cpt != 0', 8 * c + 2, c, c, 0, False, False),                       # dim % cpt == 0
            ('generic: dim/cpt = 3, not a power of two', 3 * c, c, c, 0, False, False),          # sx_pow2(dim / cpt)
            ('generic: dim/cpt = 128 > 64', 128 * c, 0, 64 * c, 0, False, False),                # dim / cpt <= 64
            ('generic: live_start % cpt != 0', 8 * c, c + 1, c, 0, False, False),                # live_start % cpt == 0
            ('generic: n_live % cpt != 0', 8 * c, c, c + 1, 0, False, False),                    # n_live % cpt == 0
            ('generic: params_stride % 4 != 0', 8 * c, c, c, 1, False, False),                   # params_stride % 4 == 0
            ('generic: live_idx list', 8 * c, 0, 2 * c, 0, True, False)]                         # live_idx == nullptr


def affine_case(n, d, l0, nl, pad, use_idx, bf, seed):
    g = gen(seed)
    xf, xs = stored(torch.randn(n, d, generator=g) * 1.5, bf)
    row = pad == 'row'
    stride = 0 if row else 2 * nl + pad
    table = torch.randn(1 if row else n, 2 * nl + (0 if row else pad), generator=g) * 0.5
    idx = torch.sort(torch.randperm(d, generator=g)[:nl]).values.to(torch.int32) if use_idx else None
    cols = idx.long() if use_idx else torch.arange(l0, l0 + nl)
    ls, shift = table[:, :nl].expand(n, nl), table[:, nl:2 * nl].expand(n, nl)
    return xf, xs, table, stride, idx, cols, ls, shift


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('row', range(len(affine_table(4))), ids=[r[0] for r in affine_table(4)])
def test_affine_coupling_dispatch(row, bf):
    """Every clause of the launcher's branch x storage type x direction x ldj absent / overwritten / accumulated x ldj_scale +-1.  bf16
    rows are processed two at a time per thread (UNR = 2): the odd row counts leave the second slot empty in the last trip."""
    name, d, l0, nl, pad, use_idx, vec = affine_table(8 if bf else 4)[row]
    C = Case('sx_affine_coupling')
    for collect in C.phases():
        for n in ROWS:
            xf, xs, table, stride, idx, cols, ls, shift = affine_case(n, d, l0, nl, pad, use_idx, bf, 100 * row + n)
            x, p, ix = put(xs), put(table), None if idx is None else put(idx)
            for reverse in (False, True):
                live32, live64 = C.cached((n, reverse), lambda: (
                    orc.affine_apply(xf[:, cols], ls, shift, reverse),
                    orc.affine_apply(xf.double()[:, cols], ls.double(), shift.double(), reverse)))
                for mode, scale in LDJ:
                    what = f'affine [{name}] {"bf16" if bf else "f32"} n={n} {"inv" if reverse else "fwd"} ldj={mode} scale={scale:+.0f}'
                    base, ldj = ldj_buffer(mode, n, gen(n))
                    y = torch.empty_like(x)
                    assert affine_vec_expected(x, y, p, stride, ix, l0, nl) == vec, what
                    if not collect:
                        affine_call(x, p, stride, ix, l0, nl, reverse, ldj, mode == 'acc', scale, y)
                    C.columns(reverse, y, x, cols, live32, live64, what)
                    C.ldj(reverse, mode, scale, ldj, base, ls.sum(-1), ls.double().sum(-1), what)


# ------------------------------------------------------------------------------------------------------------------------------
# sx_time_affine_coupling
# ------------------------------------------------------------------------------------------------------------------------------
TIME_KINDS = ('identity', 'linear', 'tanh', 'log')
# dim -> ldj_mode with an ldj buffer (sx_ldj_mode in sx_time_affine_coupling: power-of-two width <= 64 ? 1 : 2; dim 1 is a power of two there)
TIME_DIMS = {1: 1, 8: 1, 64: 1, 7: 2, 65: 2, 100: 2}


def time_call(x, params, pstride, t, tscale, kind, idx, l0, nl, reverse, ldj=None, acc=0, scale=1.0, y=None):
    n, d = x.shape
    y = torch.empty_like(x) if y is None else y
    _hip.call('sx_time_affine_coupling', x, x.data_ptr(), y.data_ptr(), _hip.ptr(ldj), params.data_ptr(), pstride, t.data_ptr(),
              _hip.ptr(tscale), kind, _hip.ptr(idx), l0, nl, n, d, _hip.dtype_code(x), int(reverse), int(acc), float(scale))
    return y


def time_refs(kind, xl, ls, shift, t, tscale, reverse, dtype):
    """(y on the live columns, the row's log-det term) in `dtype`: coupling.py:194-201 through the oracle's time embedding"""
    c = lambda v: v.to(dtype)
    layer = {'time_kind': TIME_KINDS[kind], 'time_scale': None if tscale is None else c(tscale)[None], 'time_out': 2 * ls.shape[1]}
    e_ls, e_sh = orc.time_embed(layer, c(t)[:, None]).chunk(2, dim=-1)
    lst = c(ls) * e_ls
    return orc.affine_apply(c(xl), lst, c(shift) * e_sh, reverse), lst.sum(-1)


@pytest.mark.parametrize('d', sorted(TIME_DIMS))
@pytest.mark.parametrize('kind', range(4), ids=TIME_KINDS)
def test_time_affine_coupling_dispatch(kind, d):
    """All four time nets x ldj_mode 1 / 2 x storage type x direction, the live columns as a range and as a list."""
    assert TIME_DIMS[d] == (1 if pow2(d) and d <= 64 else 2)
    nl = max(1, d // 2)
    C = Case('sx_time_affine_coupling')
    for collect in C.phases():
        for n in ROWS:
            for bf in (False, True):
                for use_idx in ((False,) if d == 1 else (False, True)):
                    g = gen(1000 * kind + 10 * d + n + bf)
                    xf, xs = stored(torch.randn(n, d, generator=g) * 1.5, bf)
                    params = torch.randn(n, 2 * nl, generator=g) * 0.5
                    t = torch.rand(n, generator=g) * 2
                    tscale = None if kind == 0 else torch.randn(2 * nl, generator=g) * 0.5
                    idx = torch.sort(torch.randperm(d, generator=g)[:nl]).values.to(torch.int32) if use_idx else None
                    l0 = d - nl
                    cols = idx.long() if use_idx else torch.arange(l0, l0 + nl)
                    x, p, td, ts, ix = put(xs), put(params), put(t), None if tscale is None else put(tscale), None if idx is None else put(idx)
                    ls, shift = params[:, :nl], params[:, nl:]
                    for reverse in (False, True):
                        (y32, l32), (y64, l64) = C.cached((n, bf, use_idx, reverse), lambda: (
                            time_refs(kind, xf[:, cols], ls, shift, t, tscale, reverse, torch.float32),
                            time_refs(kind, xf[:, cols], ls, shift, t, tscale, reverse, torch.float64)))
                        for mode, scale in (('none', 1.0), ('over', -1.0), ('acc', 1.0)):
                            what = (f'time[{TIME_KINDS[kind]}] d={d} {"bf16" if bf else "f32"} n={n} {"inv" if reverse else "fwd"} '
                                    f'{"idx" if use_idx else "range"} ldj={mode}')
                            base, ldj = ldj_buffer(mode, n, gen(n))
                            y = None if collect else time_call(x, p, 2 * nl, td, ts, kind, ix, l0, nl, reverse, ldj, mode == 'acc', scale)
                            C.columns((bf, use_idx, reverse), y, x, cols, y32, y64, what)
                            C.ldj((use_idx, reverse), mode, scale, ldj, base, l32, l64, what)


# ------------------------------------------------------------------------------------------------------------------------------
# sx_rqs_coupling / sx_cubic_coupling
# ------------------------------------------------------------------------------------------------------------------------------
LO, HI = -3.0, 3.0


def spline_call(cubic, x, params, pstride, idx, l0, nl, K, reverse, ldj=None, ldiag=None, acc=0, scale=1.0, y=None):
    n, d = x.shape
    y = torch.empty_like(x) if y is None else y
    if cubic:
        _hip.call('sx_cubic_coupling', x, x.data_ptr(), y.data_ptr(), _hip.ptr(ldj), _hip.ptr(ldiag), params.data_ptr(), pstride,
                  _hip.ptr(idx), l0, nl, K, LO, HI, n, d, _hip.dtype_code(x), int(reverse), int(acc), float(scale))
    else:
        _hip.call('sx_rqs_coupling', x, x.data_ptr(), y.data_ptr(), _hip.ptr(ldj), _hip.ptr(ldiag), params.data_ptr(), pstride,
                  _hip.ptr(idx), l0, nl, K, LO, HI, LO, HI, n, d, _hip.dtype_code(x), int(reverse), int(acc), float(scale),
                  _hip.err_flag(x.device))
    return y


def spline_P(cubic, K):
    return 2 * K + 2 if cubic else 3 * K - 1


def spline_refs(cubic, xl, table, nl, K, reverse, dtype):
    """(outputs, per-element log-derivative) of the live columns in `dtype` from the packed parameter rows"""
    P = spline_P(cubic, K)
    p3 = table[:, :nl * P].reshape(table.shape[0], nl, P).to(dtype)
    uw, uh, ud = p3[..., :K], p3[..., K:2 * K], p3[..., 2 * K:]
    f = orc.cubic_unconstrained if cubic else orc.rqs_unconstrained
    return f(xl.to(dtype), uw, uh, ud, reverse, LO, HI)


# (form, dim, live_start, n_live, live_idx?, params_stride - n_live P, ldj_mode with an ldj buffer -- sx_ldj_mode(ldj, n_live) in sx_plan_spline)
SPLINE_FORMS = [('dense 64-element spans, n_live 4', 12, 3, 4, False, 0, 1),
                ('dense 64-element spans, n_live 32', 40, 8, 32, False, 0, 1),
                ('row-aligned units, n_live 5', 12, 3, 5, False, 0, 2),
                ('row-aligned units in chunks, n_live 70', 72, 1, 70, False, 0, 2),
                ('live_idx, n_live 4', 12, 0, 4, True, 0, 1),
                ('live_idx, n_live 5', 12, 0, 5, True, 0, 2),
                ('padded parameter rows: per-element staging', 12, 3, 4, False, 3, 1)]
# rqs: K = 16 is the register path (and the LDS-DMA pipeline on whole dense spans), 17 needs the raised LDS limit (> 48 KiB per
# workgroup), 32 runs one wave per workgroup (> 64 KiB); cubic: the same thresholds sit at K = 16 (pair loads + DMA), 24 (> 48 KiB:
# 4 x 64 x 51 x 4 B) and 32 (> 64 KiB); every K takes the 16-byte staging of an aligned packed span (2K + 2 is even: cubic_kernel's staging)
SPLINE_K = {False: (1, 5, 16, 17, 32), True: (1, 5, 16, 24, 32)}


def spline_cases():
    return [pytest.param(c, f, K, id=f'{"cubic" if c else "rqs"}-K{K}-{SPLINE_FORMS[f][0]}')
            for c in (False, True) for K in SPLINE_K[c] for f in range(len(SPLINE_FORMS))]


@pytest.mark.parametrize('cubic,form,K', spline_cases())
def test_spline_coupling_dispatch(cubic, form, K):
    """Contiguous spans, the ragged last group (every row count but 64's multiples), live_idx, n_live a power of two or not, K across
    the kernels' thresholds x storage type x direction x (ldj, ldiag) absent / overwritten / accumulated.  Parameters are drawn at
    0.3 N(0, 1): bins stay off their floors and the reference's max-norm error small, so the bound is one of fp32 arithmetic."""
    name, d, l0, nl, use_idx, pad, mode_with_ldj = SPLINE_FORMS[form]
    assert mode_with_ldj == (1 if pow2(nl) and nl <= 64 else 2)
    P = spline_P(cubic, K)
    tag = 'sx_cubic_coupling' if cubic else 'sx_rqs_coupling'
    C = Case(tag)
    for collect in C.phases():
        for n in ROWS:
            g = gen(7 * K + 31 * form + n)
            table = torch.randn(n, nl * P + pad, generator=g) * 0.3
            idx = torch.sort(torch.randperm(d, generator=g)[:nl]).values.to(torch.int32) if use_idx else None
            cols = idx.long() if use_idx else torch.arange(l0, l0 + nl)
            p, ix = put(table), None if idx is None else put(idx)
            for bf in (False, True):
                xf, xs = stored(torch.randn(n, d, generator=g) * 1.6, bf)      # ~6 % of the elements in the linear tails
                x = put(xs)
                for reverse in (False, True):
                    (y32, d32), (y64, d64) = C.cached((n, bf, reverse), lambda: (
                        spline_refs(cubic, xf[:, cols], table, nl, K, reverse, torch.float32),
                        spline_refs(cubic, xf[:, cols], table, nl, K, reverse, torch.float64)))
                    for mode, scale, want_diag in (('none', 1.0, False), ('over', -1.0, True), ('acc', 1.0, False)):
                        what = f'{tag} K={K} [{name}] {"bf16" if bf else "f32"} n={n} {"inv" if reverse else "fwd"} ldj={mode} ldiag={want_diag}'
                        base, ldj = ldj_buffer(mode, n, gen(n))
                        ldiag = torch.full((n, d), float('nan'), device=DEV) if want_diag else None
                        y = None if collect else spline_call(cubic, x, p, nl * P + pad, ix, l0, nl, K, reverse, ldj, ldiag, mode == 'acc', scale)
                        C.columns((bf, reverse), y, x, cols, y32, y64, what)
                        C.ldj((bf, reverse), mode, scale, ldj, base, d32.sum(-1), d64.sum(-1), what)
                        if want_diag:
                            full32, full64 = torch.zeros(n, d), torch.zeros(n, d, dtype=torch.float64)
                            full32[:, cols], full64[:, cols] = d32, d64
                            C.store((bf, reverse, 'ldiag'), ldiag, full32, full64, what + ' ldiag')
    _hip.check_errors()


# ------------------------------------------------------------------------------------------------------------------------------
# sx_pointwise
# ------------------------------------------------------------------------------------------------------------------------------
SLOPE = 0.2
PW = {1: 'sigmoid', 2: 'logit', 3: 'elu', 4: 'elu_inv', 5: 'leaky_relu', 6: 'leaky_relu_inv'}
# dim -> (vec4 kernel?, ldj_mode with an ldj buffer): sx_pointwise's `vec4` and sx_ldj_mode (lanes per row = dim / 4 or dim; power of two <= 64 ? 1 : 2)
PW_DIMS = {8: (True, 1), 12: (True, 2), 260: (True, 2), 2: (False, 1), 7: (False, 2), 65: (False, 2)}


def pointwise_call(x, kind, param=0.0, y=None, ldj=None, ldiag=None, acc=0):
    n, d = x.shape
    _hip.call('sx_pointwise', x, x.data_ptr(), _hip.ptr(y), _hip.ptr(ldj), _hip.ptr(ldiag), n, d, _hip.dtype_code(x), kind, float(param),
              int(acc))


def pointwise_input(kind, n, d, g):
    if kind == 2:
        return torch.rand(n, d, generator=g) * 0.9 + 0.05
    if kind == 4:
        return torch.nn.functional.elu(torch.randn(n, d, generator=g) * 1.5).clamp_min(-0.96875)      # inside ELU's range (-1, inf), bf16 included
    return torch.randn(n, d, generator=g) * 2


def pointwise_refs(kind, x):
    """(out, per-element log-derivative) in x's dtype; the *_inv kinds and logit: minus the forward log-derivative at the output"""
    if kind in (1, 2):
        layer = {'kind': PW[kind]}
        return orc.pointwise_apply(layer, x, False), orc.pointwise_log_diag(layer, x)
    layer = {'kind': 'elu'} if kind in (3, 4) else {'kind': 'leaky_relu', 'negative_slope': SLOPE}
    if kind in (3, 5):
        return orc.pointwise_apply(layer, x, False), orc.pointwise_log_diag(layer, x)
    out = orc.pointwise_apply(layer, x, True)
    return out, -orc.pointwise_log_diag(layer, out)


@pytest.mark.parametrize('d', sorted(PW_DIMS))
@pytest.mark.parametrize('kind', sorted(PW), ids=[PW[k] for k in sorted(PW)])
def test_pointwise_dispatch(kind, d):
    """Every element kind in its vec4 and scalar form x the two ldj modes x ldiag present / absent x y == NULL x ldj_accumulate."""
    vec4, mode_with_ldj = PW_DIMS[d]
    lanes = d // 4 if d % 4 == 0 else d
    assert vec4 == (d % 4 == 0) and mode_with_ldj == (1 if pow2(lanes) and lanes <= 64 else 2)
    param = {5: SLOPE, 6: 1.0 / SLOPE}.get(kind, 0.0)
    C = Case('sx_pointwise')
    for collect in C.phases():
        for n in ROWS:
            for bf in (False, True):
                g = gen(100 * kind + d + n + bf)
                xf, xs = stored(pointwise_input(kind, n, d, g), bf)
                x = put(xs)
                (o32, l32), (o64, l64) = C.cached((n, bf), lambda: (pointwise_refs(kind, xf), pointwise_refs(kind, xf.double())))
                for mode, want_diag, want_y in (('none', False, True), ('over', True, True), ('acc', False, True), ('over', False, False),
                                                ('acc', True, False)):
                    what = f'pointwise[{PW[kind]}] d={d} {"bf16" if bf else "f32"} n={n} ldj={mode} ldiag={want_diag} y={want_y}'
                    base, ldj = ldj_buffer(mode, n, gen(n))
                    y = torch.empty_like(x) if want_y else None
                    ldiag = torch.full((n, d), float('nan'), device=DEV) if want_diag else None
                    if not collect:
                        pointwise_call(x, kind, param, y, ldj, ldiag, mode == 'acc')
                    if want_y:
                        C.store((bf, 'y'), y, o32, o64, what)
                    C.ldj(bf, mode, 1.0, ldj, base, l32.sum(-1), l64.sum(-1), what)
                    if want_diag:
                        C.store((bf, 'ldiag'), ldiag, l32, l64, what + ' ldiag')


# (kernel, storage, dim): sx_pointwise's cumsum / diff branch (fp32, dim % 4 == 0, aligned -> 16-byte kernels; dim <= 64 -> the pipelined one)
CUMSUM = [('cumsum_vec_pipe_kernel', False, 8), ('cumsum_vec_pipe_kernel', False, 64), ('cumsum_vec_kernel', False, 68),
          ('cumsum_kernel', False, 7), ('cumsum_kernel', True, 8), ('cumsum_kernel', True, 7)]


@pytest.mark.parametrize('diff', [False, True], ids=['cumsum', 'diff'])
@pytest.mark.parametrize('kernel,bf,d', CUMSUM, ids=[f'{k}-{"bf16" if b else "f32"}-{d}' for k, b, d in CUMSUM])
def test_cumsum_diff_dispatch(kernel, bf, d, diff):
    """Cumsum / Diff in their three kernels; the log-det outputs are zeros (overwritten) or left as they were (accumulated)."""
    vec = (not bf) and d % 4 == 0
    assert kernel == ('cumsum_kernel' if not vec else 'cumsum_vec_pipe_kernel' if d <= 64 else 'cumsum_vec_kernel')
    layer = {'kind': 'diff' if diff else 'cumsum'}
    C = Case('sx_pointwise')
    for collect in C.phases():
        for n in ROWS:
            xf, xs = stored(torch.randn(n, d, generator=gen(d + n)) * 2, bf)
            x = put(xs)
            for mode in ('none', 'over', 'acc'):
                what = f'{layer["kind"]} [{kernel}] {"bf16" if bf else "f32"} d={d} n={n} ldj={mode}'
                base, ldj = ldj_buffer(mode, n, gen(n))
                y = torch.empty_like(x)
                ldiag = torch.full((n, d), float('nan'), device=DEV) if mode == 'over' else None
                if not collect:
                    pointwise_call(x, 8 if diff else 7, 0.0, y, ldj, ldiag, mode == 'acc')
                C.store('y', y, orc.pointwise_apply(layer, xf, False), orc.pointwise_apply(layer, xf.double(), False), what)
                if not collect and mode != 'none':
                    assert torch.equal(ldj.cpu(), base if mode == 'acc' else torch.zeros(n)), what
                if not collect and ldiag is not None:
                    assert torch.equal(ldiag.cpu(), torch.zeros(n, d)), what


# ------------------------------------------------------------------------------------------------------------------------------
# sx_unit_normal_logprob
# ------------------------------------------------------------------------------------------------------------------------------
# (dim, bf16) -> kernel: sx_unit_normal_logprob (bf16x8: dim / 8 a power of two <= 64; vec4: dim / 4 a power of two <= 64)
NORMAL = {(1, False): 'generic', (4, False): 'vec4', (8, False): 'vec4', (12, False): 'generic', (256, False): 'vec4',
          (260, False): 'generic', (512, False): 'generic',
          (1, True): 'generic', (4, True): 'vec4', (8, True): 'bf16x8', (12, True): 'generic', (256, True): 'bf16x8',
          (260, True): 'generic', (512, True): 'bf16x8'}


def normal_kernel(d, bf, ptr=0):
    if bf and d % 8 == 0 and pow2(d // 8) and d // 8 <= 64 and ptr % 16 == 0:
        return 'bf16x8'
    return 'vec4' if d % 4 == 0 and pow2(d // 4) and d // 4 <= 64 and ptr % 16 == 0 else 'generic'


def UNIT(d):
    return st.UnitNormal(d).to(DEV)


def normal_call(x, ldj=None):
    out = torch.full((x.shape[0],), float('nan'), device=DEV)
    _hip.call('sx_unit_normal_logprob', x, x.data_ptr(), _hip.ptr(ldj), out.data_ptr(), x.shape[0], x.shape[1], _hip.dtype_code(x))
    return out


@pytest.mark.parametrize('d,bf', sorted(NORMAL), ids=[f'{d}-{"bf16" if b else "f32"}' for d, b in sorted(NORMAL)])
def test_unit_normal_dispatch(d, bf):
    C = Case('sx_unit_normal_logprob')
    for collect in C.phases():
        for n in ROWS:
            g = gen(d + n)
            xf, xs = stored(torch.randn(n, d, generator=g), bf)
            x = put(xs)
            assert normal_kernel(d, bf, x.data_ptr()) == NORMAL[(d, bf)]
            for with_ldj in (False, True):
                l = torch.randn(n, generator=g) * 3 if with_ldj else None
                got = None if collect else normal_call(x, None if l is None else put(l))
                r32 = orc.unit_normal_log_prob(xf) + (l if with_ldj else 0)
                r64 = orc.unit_normal_log_prob(xf.double()) + (l.double() if with_ldj else 0)
                C.store(with_ldj, got, r32, r64, f'unit_normal [{NORMAL[(d, bf)]}] d={d} {"bf16" if bf else "f32"} n={n} ldj={with_ldj}')


# ------------------------------------------------------------------------------------------------------------------------------
# sx_permute
# ------------------------------------------------------------------------------------------------------------------------------
# row bytes -> kernel: sx_permute (rows of a multiple of 16 bytes that divide 4096 go through LDS)
PERMUTE = {16: 'lds', 4096: 'lds', 48: 'plain', 4112: 'plain'}


def permute_call(x, idx, y=None):
    y = torch.empty_like(x) if y is None else y
    _hip.call('sx_permute', x, x.data_ptr(), y.data_ptr(), idx.data_ptr(), x.shape[0], x.shape[1], x.element_size())
    return y


def permute_lds_expected(x, y):
    rb = x.shape[1] * x.element_size()
    return rb % 16 == 0 and rb <= 4096 and 4096 % rb == 0 and x.shape[1] <= 2048 and (x.data_ptr() | y.data_ptr()) % 16 == 0


@pytest.mark.parametrize('row_bytes', sorted(PERMUTE))
@pytest.mark.parametrize('elem', [2, 4])
def test_permute_dispatch(elem, row_bytes):
    """Random bit patterns (NaNs, infinities and subnormals among them) moved by a random permutation: bit-exact."""
    d = row_bytes // elem
    dt = torch.int16 if elem == 2 else torch.int32
    for n in ROWS:
        g = gen(row_bytes + n)
        xs = torch.randint(-2 ** 15, 2 ** 15, (n, d), generator=g).to(dt) if elem == 2 else \
            torch.randint(-2 ** 31, 2 ** 31, (n, d), generator=g, dtype=torch.int64).to(dt)
        perm = torch.randperm(d, generator=g)
        x, y = put(xs), torch.empty(n, d, dtype=dt, device=DEV)
        assert permute_lds_expected(x, y) == (PERMUTE[row_bytes] == 'lds')
        permute_call(x, put(perm.to(torch.int32)), y)
        assert torch.equal(y.cpu(), xs[:, perm]), (elem, row_bytes, n)


# ------------------------------------------------------------------------------------------------------------------------------
# exact rounding ties and special values
# ------------------------------------------------------------------------------------------------------------------------------
def tie_rows():
    """(x, shift) with x + shift exact in fp32 and on (or just beside) a bf16 rounding tie: round-to-nearest-even takes 1 + 2^-8 to 1,
    1 + 2^-7 + 2^-8 to 1 + 2^-6 and 3 + 2^-7 to 3; their negatives mirror; one fp32 ulp beyond a tie rounds away from it."""
    e = lambda k: 2.0 ** k
    x = torch.tensor([1.0, 1.0, -1.0, -1.0, 3.0, -3.0, 1.0, 1.0])
    s = torch.tensor([e(-8), e(-7) + e(-8), -e(-8), -(e(-7) + e(-8)), e(-7), -e(-7), e(-8) + e(-16), e(-8) - e(-16)])
    want = torch.tensor([1.0, 1 + e(-6), -1.0, -(1 + e(-6)), 3.0, -3.0, 1 + e(-7), 1.0])
    assert torch.equal((x + s).bfloat16().float(), want)           # torch's CPU conversion rounds to nearest even
    assert torch.equal(x.bfloat16().float(), x)
    return x, s


@pytest.mark.parametrize('kernel', ['vec', 'generic'])
def test_affine_kernel_rounds_ties_to_even(kernel):
    """log_scale = 0, shifts that put x + shift on a tie: bit-exact against torch's CPU .bfloat16() of the exact fp32 sum, in the vec
    kernel and in the generic one (a live_idx list), both directions."""
    x1, s1 = tie_rows()
    for n in (1, 63, 130):
        x = x1.repeat(n, 1)
        x[1::2] = -x[1::2]
        s = s1.repeat(n, 1)
        s[1::2] = -s[1::2]
        want = bits((x + s).bfloat16())
        xd = put(x.bfloat16())
        idx = put(torch.arange(8, dtype=torch.int32)) if kernel == 'generic' else None
        for reverse in (False, True):
            params = torch.cat([torch.zeros(n, 8), -s if reverse else s], -1)
            p = put(params)
            y = torch.empty_like(xd)
            assert affine_vec_expected(xd, y, p, 16, idx, 0, 8) == (kernel == 'vec')
            affine_call(xd, p, 16, idx, 0, 8, reverse, y=y)
            assert torch.equal(bits(y), want), (kernel, n, reverse)


def tie_flow(flip):
    """One fused affine coupling (D = 64, hidden 64) whose conditioner's last Linear has a zero weight: its bias alone sets
    log_scale = 0 and the shift, here the tie shifts on the 32 transformed columns."""
    torch.manual_seed(0)
    desc = fd.cfg2_desc(1, 64, 64) + ([{'kind': 'flip'}] if flip else [])
    flow = fd.build_flow(st, desc, 64)
    last = flow.transforms[0].transform.latent_net.net[-1]
    x1, s1 = tie_rows()
    live = torch.nonzero(orc.mask_vector('ordered_right_half', 64) == 0).flatten()
    assert live.numel() == 32
    shift = torch.zeros(64)
    shift[live] = s1.repeat(4)
    last.weight.zero_()
    last.bias.copy_(torch.cat([torch.zeros(64), shift]))
    xrow = torch.randn(64).bfloat16().float()
    xrow[live] = x1.repeat(4)
    return flow.to(DEV), xrow, shift, live


@pytest.mark.parametrize('flip', [False, True], ids=['identity_cols', 'gathered'])
def test_fused_coupling_rounds_ties_to_even(flip):
    """The same ties through the fused kernel's y store: the identity_cols vector form and, behind a Flip, the gathered-columns form.
    exp2(0) = 1, the zero weight contributes exact zeros to the MFMA accumulators and the bias is carried in fp32, so x + shift is
    exact before the store."""
    flow, xrow, shift, live = tie_flow(flip)
    prog = flow._fused_program(False, 64, 0, torch.device(DEV, 0))
    assert prog is not None and bool(prog.prog.identity_cols) == (not flip)
    for n in (1, 63, 257):
        x = xrow.repeat(n, 1)
        want = (x + shift).bfloat16()                          # pass-through columns: + 0, their bits kept
        if flip:
            want = torch.flip(want, [-1])
        y = flow.forward(put(x.bfloat16()))
        assert y.dtype == torch.bfloat16
        assert torch.equal(bits(y), bits(want)), (flip, n)


SPECIAL_BITS = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x8001, 0x007F, 0x7F7F, 0xFF7F, 0x3F80, 0xC040]
# +0, -0, +Inf, -Inf, NaN, the smallest and the largest bf16 subnormals, the largest finite bf16 (+-), 1, -3


def special_block(n, d, bf):
    """[n, d] in the storage type: the special values cycled through every column (bf16 bit patterns; the same values in fp32)"""
    pat = torch.tensor([b - 65536 if b >= 32768 else b for b in SPECIAL_BITS], dtype=torch.int16)
    v = pat.repeat((n * d + len(pat) - 1) // len(pat))[:n * d].reshape(n, d).view(torch.bfloat16)
    return v if bf else v.float()


def same_bits_nan_aware(got, want):
    g, w = got.cpu(), want.cpu()
    nan = torch.isnan(w.float())
    return torch.equal(torch.isnan(g.float()), nan) and torch.equal(bits(g)[~nan], bits(w)[~nan])


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
def test_special_values_in_pass_through_columns(bf):
    """+-0, +-Inf, NaN, subnormals and the largest finite value in the columns a coupling kernel copies: bits kept, NaN stays NaN."""
    c = 8 if bf else 4
    for n in (1, 63, 257):
        g = gen(n)
        for name, d, l0, nl in (('affine vec', 8 * c, 4 * c, 4 * c), ('affine generic', 8 * c + 1, 3, 5)):
            x = special_block(n, d, bf)
            x[:, l0:l0 + nl] = torch.randn(n, nl, generator=g).to(x.dtype)
            xd, p = put(x), put(torch.randn(n, 2 * nl, generator=g) * 0.5)
            y = affine_call(xd, p, 2 * nl, None, l0, nl, False)
            rest = [j for j in range(d) if not l0 <= j < l0 + nl]
            assert same_bits_nan_aware(y[:, rest], xd[:, rest]), (name, n)
            assert torch.isfinite(y[:, l0:l0 + nl].float()).all(), (name, n)
        d, l0, nl = 12, 3, 4
        x = special_block(n, d, bf)
        x[:, l0:l0 + nl] = (torch.randn(n, nl, generator=g) * 1.5).to(x.dtype)
        xd = put(x)
        rest = [j for j in range(d) if not l0 <= j < l0 + nl]
        t, ts = put(torch.rand(n, generator=g)), put(torch.randn(2 * nl, generator=g))
        y = time_call(xd, put(torch.randn(n, 2 * nl, generator=g) * 0.5), 2 * nl, t, ts, 2, None, l0, nl, False)
        assert same_bits_nan_aware(y[:, rest], xd[:, rest]), ('time', n)
        for cubic in (False, True):
            K = 5
            p = put(torch.randn(n, nl * spline_P(cubic, K), generator=g) * 0.3)
            ldiag = torch.full((n, d), float('nan'), device=DEV)
            y = spline_call(cubic, xd, p, nl * spline_P(cubic, K), None, l0, nl, K, False, None, ldiag)
            assert same_bits_nan_aware(y[:, rest], xd[:, rest]), ('cubic' if cubic else 'rqs', n)
            assert torch.equal(ldiag[:, rest].cpu(), torch.zeros(n, len(rest))) and torch.isfinite(ldiag).all()
    _hip.check_errors()


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
def test_special_values_through_permute_and_flip(bf):
    for d in (8, 12):                                            # LDS form (fp32: 32 B, bf16: 16 B rows) and plain form
        x = special_block(63, d, bf)
        xd = put(x)
        p = st.Permute(d).to(DEV)
        perm = p.permutation.cpu().long()
        assert torch.equal(bits(p(xd)), bits(x[:, perm]))
        assert torch.equal(bits(p.inverse(p(xd))), bits(x))
        assert torch.equal(bits(st.Flip([-1])(xd)), bits(torch.flip(x, [-1])))


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
def test_special_values_through_unit_normal(bf):
    """One special value per row among ordinary ones: the fp32 result of every row whose fp32 reference is finite meets the fp32
    bound of the fp64 value of the upcast input; the others (+-Inf and the largest finite value, whose square leaves fp32: -inf; NaN:
    NaN) come back as the reference's own non-finite value, in their own rows only."""
    for d in (8, 4, 12, 5):                                      # bf16x8 / vec4 (8, 4), generic (12, 5)
        n = 4 * len(SPECIAL_BITS) + 1
        g = gen(d)
        x = torch.randn(n, d, generator=g).bfloat16()
        sp = special_block(1, len(SPECIAL_BITS), True).flatten()
        for i, v in enumerate(sp):
            x[4 * i + 1, i % d] = v
        xs = x if bf else x.float()
        got = UNIT(d).log_prob(put(xs)).cpu()
        r32, r64 = orc.unit_normal_log_prob(x.float()), orc.unit_normal_log_prob(x.double())
        fin = torch.isfinite(r32)
        assert int((~fin).sum()) == 5 and torch.equal(torch.isfinite(got), fin)
        assert torch.equal(torch.isnan(got), torch.isnan(r32)) and torch.equal(got[~fin & ~torch.isnan(r32)], r32[~fin & ~torch.isnan(r32)])
        assert_f32(got[fin], r32[fin], r64[fin], f'unit_normal special values d={d} {"bf16" if bf else "f32"}', 'sx_unit_normal_logprob')



# ------------------------------------------------------------------------------------------------------------------------------
# offset views: base pointers that are element-aligned only
#
# What each launcher does with such a pointer, read from the code before any of this ran:
#   sx_affine_coupling       x, y, params tested in its `fast` condition -> generic kernel (element accesses); ldj: elements
#   sx_time_affine_coupling  element accesses only
#   sx_rqs / sx_cubic        x, y, ldiag, ldj: element accesses; params: 16-byte staging / LDS-DMA only behind
#                            (params & 15) == 0 (rqs_kernel's `contig`, cubic_kernel's `lin` and vector staging), else per-element staging
#   sx_pointwise             x, y tested against 4 elements and ldiag against 16 bytes in its `vec4` condition -> scalar kernel;
#                            cumsum / diff: x | y tested before the 16-byte kernels -> cumsum_kernel
#   sx_unit_normal_logprob   x tested by both vector branches -> generic kernel; ldj, out: elements
#   sx_permute               x | y tested by the LDS branch -> plain kernel
#   sx_flow_run2             identity_cols programs load x / store y as 16-byte (fp32) or 8-byte (bf16) vectors; x is REJECTED
#                            unless 16-byte aligned (sx_flow_fused.hip:314) -- the binding copies (fused.needs_aligned_copy); y is the
#                            binding's own allocation; latent and the gathered-columns form: element accesses
#   sx_cnf_flow / sx_resnet_flow   x, y, latent: element accesses
# No entry point issues an access wider than the alignment it has checked.
# ------------------------------------------------------------------------------------------------------------------------------
def offsets(bf):
    return (1, 2, 4) if bf else (1,)


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('which', ['x', 'y', 'params', 'ldj'])
def test_affine_coupling_offset_pointers(which, bf):
    """A shape that takes the vec kernel when aligned, with one pointer offset at a time (x through the Python wrapper)."""
    from stribor_amd.flows.affine import run_affine_kernel
    c = 8 if bf else 4
    n, d, l0, nl = 257, 8 * c, 4 * c, 4 * c
    xf, xs, table, stride, _, cols, ls, shift = affine_case(n, d, l0, nl, 0, False, bf, 5)
    for k in (offsets(bf) if which in ('x', 'y') else (1,)):
        for reverse in (False, True):
            what = f'affine offset {which}+{k} {"bf16" if bf else "f32"} {"inv" if reverse else "fwd"}'
            live32 = orc.affine_apply(xf[:, cols], ls, shift, reverse)
            live64 = orc.affine_apply(xf.double()[:, cols], ls.double(), shift.double(), reverse)
            x, p = put(xs, k if which == 'x' else 0), put(table, k if which == 'params' else 0)
            if which == 'x':
                y, ldj = run_affine_kernel(x, p, stride, None, l0, nl, reverse, True, True, -1.0)
            else:
                y = put(torch.zeros_like(xs), k if which == 'y' else 0)
                ldj = put(torch.zeros(n), k if which == 'ldj' else 0)
                assert affine_vec_expected(x, y, p, stride, None, l0, nl) == (which == 'ldj')
                affine_call(x, p, stride, None, l0, nl, reverse, ldj, 0, -1.0, y)
            check_columns(y, x, cols, live32, live64, what, 'sx_affine_coupling')
            assert_f32(ldj, -ls.sum(-1), -ls.double().sum(-1), what + ' ldj', 'sx_affine_coupling')


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('which', ['x', 'y', 'params', 'ldj', 't'])
def test_time_affine_coupling_offset_pointers(which, bf):
    n, d, nl, kind = 257, 8, 4, 2
    g = gen(11)
    xf, xs = stored(torch.randn(n, d, generator=g) * 1.5, bf)
    params, t, tscale = torch.randn(n, 2 * nl, generator=g) * 0.5, torch.rand(n, generator=g) * 2, torch.randn(2 * nl, generator=g) * 0.5
    cols = torch.arange(4, 8)
    y32, l32 = time_refs(kind, xf[:, cols], params[:, :nl], params[:, nl:], t, tscale, False, torch.float32)
    y64, l64 = time_refs(kind, xf[:, cols], params[:, :nl], params[:, nl:], t, tscale, False, torch.float64)
    for k in (offsets(bf) if which in ('x', 'y') else (1,)):
        x = put(xs, k if which == 'x' else 0)
        y = put(torch.zeros_like(xs), k if which == 'y' else 0)
        ldj = put(torch.zeros(n), k if which == 'ldj' else 0)
        time_call(x, put(params, k if which == 'params' else 0), 2 * nl, put(t, k if which == 't' else 0), put(tscale), kind, None, 4, nl,
                  False, ldj, 0, 1.0, y)
        what = f'time offset {which}+{k} {"bf16" if bf else "f32"}'
        check_columns(y, x, cols, y32, y64, what, 'sx_time_affine_coupling')
        assert_f32(ldj, l32, l64, what + ' ldj', 'sx_time_affine_coupling')


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('which', ['x', 'y', 'params', 'ldj', 'ldiag'])
@pytest.mark.parametrize('cubic', [False, True], ids=['rqs', 'cubic'])
def test_spline_coupling_offset_pointers(cubic, which, bf):
    """K = 16 on whole dense spans: aligned parameters are streamed by LDS-DMA, offset ones staged element by element."""
    from stribor_amd.flows.spline import run_cubic_kernel, run_rqs_kernel
    n, d, l0, nl, K = 257, 40, 8, 32, 16
    P = spline_P(cubic, K)
    tag = 'sx_cubic_coupling' if cubic else 'sx_rqs_coupling'
    g = gen(13)
    table = torch.randn(n, nl * P, generator=g) * 0.3
    xf, xs = stored(torch.randn(n, d, generator=g) * 1.6, bf)
    cols = torch.arange(l0, l0 + nl)
    for k in (offsets(bf) if which in ('x', 'y') else (1,)):
        for reverse in (False, True):
            y32, d32 = spline_refs(cubic, xf[:, cols], table, nl, K, reverse, torch.float32)
            y64, d64 = spline_refs(cubic, xf[:, cols], table, nl, K, reverse, torch.float64)
            what = f'{tag} offset {which}+{k} {"bf16" if bf else "f32"} {"inv" if reverse else "fwd"}'
            x, p = put(xs, k if which == 'x' else 0), put(table, k if which == 'params' else 0)
            if which == 'x':
                if cubic:
                    y, ldj, ldiag = run_cubic_kernel(x, p, nl * P, None, l0, nl, K, LO, HI, reverse, True, True)
                else:
                    y, ldj, ldiag = run_rqs_kernel(x, p, nl * P, None, l0, nl, K, LO, HI, LO, HI, reverse, True, True)
            else:
                y = put(torch.zeros_like(xs), k if which == 'y' else 0)
                ldj = put(torch.zeros(n), k if which == 'ldj' else 0)
                ldiag = put(torch.full((n, d), float('nan')), k if which == 'ldiag' else 0)
                spline_call(cubic, x, p, nl * P, None, l0, nl, K, reverse, ldj, ldiag, 0, 1.0, y)
            check_columns(y, x, cols, y32, y64, what, tag)
            assert_f32(ldj, d32.sum(-1), d64.sum(-1), what + ' ldj', tag)
            full32, full64 = torch.zeros(n, d), torch.zeros(n, d, dtype=torch.float64)
            full32[:, cols], full64[:, cols] = d32, d64
            assert_f32(ldiag, full32, full64, what + ' ldiag', tag)
    _hip.check_errors()


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('which', ['x', 'y', 'ldj', 'ldiag'])
def test_pointwise_offset_pointers(which, bf):
    """dim 8 takes the vec4 kernel when aligned; cumsum at dim 8 the pipelined 16-byte kernel (fp32)."""
    from stribor_amd.flows.pointwise import run_pointwise
    n, d = 257, 8
    for kind in (1, 3, 7):
        g = gen(17 + kind)
        xf, xs = stored(torch.randn(n, d, generator=g) * 2, bf)
        if kind == 7:
            o32, o64 = xf.cumsum(-1), xf.double().cumsum(-1)
            l32, l64 = torch.zeros(n, d), torch.zeros(n, d, dtype=torch.float64)
        else:
            (o32, l32), (o64, l64) = pointwise_refs(kind, xf), pointwise_refs(kind, xf.double())
        for k in (offsets(bf) if which in ('x', 'y') else (1,)):
            what = f'pointwise kind {kind} offset {which}+{k} {"bf16" if bf else "f32"}'
            x = put(xs, k if which == 'x' else 0)
            if which == 'x':
                y, ldj, ldiag = run_pointwise(x, kind, 0.0, True, True, True)
                ldj = ldj.reshape(-1)
            else:
                y = put(torch.zeros_like(xs), k if which == 'y' else 0)
                ldj = put(torch.full((n,), float('nan')), k if which == 'ldj' else 0)
                ldiag = put(torch.full((n, d), float('nan')), k if which == 'ldiag' else 0)
                pointwise_call(x, kind, 0.0, y, ldj, ldiag, 0)
            assert_store(y, o32, o64, what, 'sx_pointwise')
            assert_f32(ldj, l32.sum(-1), l64.sum(-1), what + ' ldj', 'sx_pointwise')
            assert_f32(ldiag, l32, l64, what + ' ldiag', 'sx_pointwise')


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('which', ['x', 'ldj', 'out'])
def test_unit_normal_offset_pointers(which, bf):
    n = 257
    for d in (8, 256):
        g = gen(d)
        xf, xs = stored(torch.randn(n, d, generator=g), bf)
        l = torch.randn(n, generator=g)
        r32, r64 = orc.unit_normal_log_prob(xf), orc.unit_normal_log_prob(xf.double())
        for k in (offsets(bf) if which == 'x' else (1,)):
            what = f'unit_normal offset {which}+{k} d={d} {"bf16" if bf else "f32"}'
            if which == 'x':
                x = put(xs, k)
                assert normal_kernel(d, bf, x.data_ptr()) == 'generic'
                assert_f32(UNIT(d).log_prob(x), r32, r64, what, 'sx_unit_normal_logprob')
            else:
                x = put(xs)
                out = put(torch.full((n,), float('nan')), 1 if which == 'out' else 0)
                _hip.call('sx_unit_normal_logprob', x, x.data_ptr(), put(l, 1 if which == 'ldj' else 0).data_ptr(), out.data_ptr(), n, d,
                          _hip.dtype_code(x))
                assert_f32(out, r32 + l, r64 + l.double(), what, 'sx_unit_normal_logprob')


@pytest.mark.parametrize('elem', [2, 4])
@pytest.mark.parametrize('which', ['x', 'y'])
def test_permute_offset_pointers(which, elem):
    """Rows of 16 and 4096 bytes go through LDS when aligned; offset by one element (and 2, 4 for 2-byte elements) they must take the
    plain kernel and still move every bit (x through the Permute module, y through the C ABI)."""
    for row_bytes in (16, 4096):
        d, n = row_bytes // elem, 63
        dt = torch.bfloat16 if elem == 2 else torch.float32
        xs = special_block(n, d, True) if elem == 2 else torch.randn(n, d, generator=gen(d))
        p = st.Permute(d).to(DEV)
        perm = p.permutation.cpu().long()
        for k in offsets(elem == 2):
            if which == 'x':
                y = p(put(xs, k))
            else:
                x, y = put(xs), put(torch.zeros(n, d, dtype=dt), k)
                assert not permute_lds_expected(x, y)
                permute_call(x, put(perm.to(torch.int32)), y)
            assert torch.equal(bits(y), bits(xs[:, perm])), (which, elem, row_bytes, k)


def flow_case(desc, dim, latent_dim=0, seed=0):
    torch.manual_seed(seed)
    flow = fd.build_flow(st, desc, dim)
    spec = fd.flow_spec(desc, {k: v.clone() for k, v in flow.state_dict().items()})
    return flow.to(DEV), spec, orc.spec_to(spec, torch.float64)


def check_flow_offsets(flow, spec, spec64, xf, xs, ks, lat=None, lat_k=0, what=''):
    """log_prob, inverse and forward of an offset x (and latent): the call returns and meets the fp64 bound the aligned call meets."""
    kw32 = {} if lat is None else {'latent': lat}
    kw64 = {} if lat is None else {'latent': lat.double()}
    refs = {'log_prob': (orc.flow_log_prob(spec, xf, **kw32), orc.flow_log_prob(spec64, xf.double(), **kw64)),
            'inverse': (orc.flow_inverse(spec, xf, **kw32), orc.flow_inverse(spec64, xf.double(), **kw64)),
            'forward': (orc.flow_forward(spec, xf, **kw32), orc.flow_forward(spec64, xf.double(), **kw64))}
    for name, (r32, r64) in refs.items():
        kw = {} if lat is None else {'latent': put(lat)}
        aligned = getattr(flow, name)(put(xs), **kw)
        assert_store(aligned, r32, r64, f'{what} {name} aligned', 'sx_flow_run2')
        for k in ks:
            kw = {} if lat is None else {'latent': put(lat, lat_k)}
            x = put(xs, k)
            assert x.data_ptr() % 16 != 0
            assert_store(getattr(flow, name)(x, **kw), r32, r64, f'{what} {name} x+{k}', 'sx_flow_run2')


@pytest.mark.parametrize('bf', [False, True], ids=['f32', 'bf16'])
def test_fused_flow_offset_x(bf):
    """cfg 2 at D = 64 with two layers (an identity_cols program): sx_flow_run2 rejects an x that is not 16-byte aligned, the binding
    hands it an aligned copy."""
    flow, spec, spec64 = flow_case(fd.cfg2_desc(2, 64, 64), 64)
    prog = flow._fused_program(True, 64, 0, torch.device(DEV, 0))
    assert prog is not None and prog.prog.identity_cols == 1
    xf, xs = stored(torch.randn(257, 64, generator=gen(3)), bf)
    check_flow_offsets(flow, spec, spec64, xf, xs, offsets(bf), what=f'cfg2 {"bf16" if bf else "f32"}')


def test_fused_flow_bf16_dim12_row_slice():
    """bf16 rows of 24 bytes: x[1:] starts 8 bytes past a 16-byte boundary."""
    flow, spec, spec64 = flow_case(fd.cfg2_desc(2, 12, 32), 12, seed=1)
    assert flow._fused_program(True, 12, 0, torch.device(DEV, 0)).prog.identity_cols == 1
    xb = torch.randn(101, 12, generator=gen(4)).bfloat16()
    big = put(xb)
    view = big[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    xf = xb[1:].float()
    for name, f32, args in (('log_prob', orc.flow_log_prob, {}), ('inverse', orc.flow_inverse, {}), ('forward', orc.flow_forward, {})):
        got = getattr(flow, name)(view)
        assert torch.equal(bits(got), bits(getattr(flow, name)(put(xb[1:]))))
        assert_store(got, f32(spec, xf), f32(spec64, xf.double()), f'dim 12 bf16 x[1:] {name}', 'sx_flow_run2')


def test_fused_flow_offset_latent():
    """Two couplings over 32 columns with a 3-column latent (one data tile + one latent tile: a fused identity_cols program; at 64
    columns such a flow runs layer by layer): the latent is read element by element, offset by one float and by its own row."""
    desc = [{'kind': 'coupling_affine', 'dim': 32, 'hidden': [64], 'mask': m, 'latent_dim': 3}
            for m in ('ordered_right_half', 'ordered_left_half')]
    flow, spec, spec64 = flow_case(desc, 32, 3, seed=2)
    prog = flow._fused_program(True, 32, 3, torch.device(DEV, 0))
    assert prog is not None and prog.prog.identity_cols == 1 and prog.prog.latent_dim == 3
    g = gen(5)
    xf, lat = torch.randn(257, 32, generator=g), torch.randn(257, 3, generator=g)
    check_flow_offsets(flow, spec, spec64, xf, xf, (1,), lat, 1, 'couplings + latent')
    check_flow_offsets(flow, spec, spec64, xf, xf, (1,), lat, 3, 'couplings + latent (latent one row in)')


def test_fused_spline_flow_offset_x():
    flow, spec, spec64 = flow_case(fd.cfg3_desc(2, 8, 32, 5), 8, seed=3)
    assert flow._fused_program(True, 8, 0, torch.device(DEV, 0)) is not None
    xf = torch.randn(257, 8, generator=gen(6)) * 1.5
    check_flow_offsets(flow, spec, spec64, xf, xf, (1,), what='spline flow')
    _hip.check_errors()


def test_fused_flip_relabelled_flow_offset_x():
    """A Flip between the couplings relabels the columns: the gathered-columns form, which takes any element-aligned x."""
    c = fd.cfg2_desc(2, 64, 64)
    flow, spec, spec64 = flow_case([c[0], {'kind': 'flip'}, c[1]], 64, seed=4)
    prog = flow._fused_program(True, 64, 0, torch.device(DEV, 0))
    assert prog is not None and prog.prog.identity_cols == 0
    for bf in (False, True):
        xf, xs = stored(torch.randn(257, 64, generator=gen(7)), bf)
        check_flow_offsets(flow, spec, spec64, xf, xs, offsets(bf), what=f'flip flow {"bf16" if bf else "f32"}')


def test_continuous_transform_offset_x():
    """sx_cnf_flow (DiffeqMLP, dim 5) reads x element by element: same bits as the aligned call, which meets the fp64 bound."""
    case = 'grid/7x4x5/h1/rk4/s1/T1.0/l0'
    f, x, lat, m = ch.build_case(case)
    y64, l64 = ch.solve64(f, x, lat)
    f = f.to(DEV)
    y, l = f.forward_and_log_det_jacobian(put(x))
    assert f._last_path == 'kernel'
    yo, lo = f.forward_and_log_det_jacobian(put(x.reshape(-1, 5), 1).view(x.shape))
    assert f._last_path == 'kernel'
    assert torch.equal(yo, y) and torch.equal(lo, l)
    assert_f32(y, ch.golden().t(f'{case}/y'), y64, 'cnf y', 'sx_cnf_flow')
    assert_f32(l, ch.golden().t(f'{case}/ldj'), l64, 'cnf ldj', 'sx_cnf_flow')


def test_iresnet_offset_x():
    """sx_resnet_flow reads x element by element: forward and the fixed-point inverse of an offset x equal the aligned call's."""
    torch.manual_seed(5)
    f = fd.build_transform(st, {'kind': 'iresnet', 'dim': 5, 'hidden': [32, 32]}).to(DEV).train()
    for _ in range(5):                     # the power iteration settles (a fresh u, v under-estimates the Lipschitz constant)
        f(torch.randn(16, 5, device=DEV))
    f.eval()
    x = torch.randn(257, 5, generator=gen(8))
    y = f(put(x))
    assert torch.isfinite(y).all() and torch.equal(f(put(x, 1)), y)
    xb = f.inverse(y)
    assert torch.isfinite(xb).all() and torch.equal(f.inverse(offset_view(y, 1)), xb)


def test_continuous_affine_coupling_offset_x():
    """The module path of sx_time_affine_coupling: its conditioner is an MLP program (identity_cols) that sees the same offset x."""
    torch.manual_seed(6)
    f = fd.build_transform(st, {'kind': 'continuous_affine_coupling', 'dim': 8, 'hidden': [16], 'mask': 'ordered_right_half',
                                'time_kind': 'tanh'}).to(DEV)
    g = gen(9)
    x, t = torch.randn(257, 8, generator=g), torch.rand(257, 1, generator=g)
    y = f(put(x), t=put(t))
    assert torch.isfinite(y).all() and torch.equal(f(put(x, 1), t=put(t)), y)


def test_zz_worst_ratios():
    """Not a check of its own: prints the largest err / bound (fp32) and err / (ulp/2 + bound) (bf16) every launcher reached in the
    tests of this module that ran before it."""
    for (launcher, kind), r in sorted(WORST.items()):
        print(f'WORST {launcher} {kind} {r:.3f}')
    assert all(r <= 1.0 for r in WORST.values())
