"""The cases of tests/golden/f26_spline_parent_bits.npz, shared by tools/make_spline_parent_bits.py (which records what the library it
is run against produces) and tests/test_gpu_spline_parent_bits.py (which holds later builds to those bits): every kernel that reads
the spline arithmetic of stribor_amd/csrc/sx_rqs_core.h, sx_cubic_core.h and the transcendental helpers of sx_common.h -- the
stand-alone spline kernels and their backwards, the one-launch spline flows in both arithmetics, the slab forward tier, one training
step through the slab backward, and the point-wise kernels whose exp / log are those helpers.

A case is a function -> {name: tensor}; every row output and log-det is stored whole.  The launch wrappers and flow builders are
those of the kernels' own test modules and of the package (imported, not restated).  129 rows (two workgroups, a ragged last row
group), width 8, conditioner hidden width 16 unless the case says otherwise.  Only the stand-alone kernels' grids are capped by the
device's CU count, far above what these sizes launch: no case here depends on it (CU_CASES is empty), the meta records it all the same."""
import torch

import flowdesc as fd
import test_gpu_storage as tgs

import stribor_amd as st
from stribor_amd.flows import spline as sp

DEV = 'cuda'
ROWS = 129
DIM = 8
HIDDEN = 16
LO, HI = tgs.LO, tgs.HI


def _gen(tag):
    return torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(tag)))


# ---- sx_rqs_coupling / sx_cubic_coupling ----------------------------------------------------------------------------------------------
def _coupling(cubic, K, reverse, bf, rows=37, d=12, l0=3, nl=8):
    """rows x nl elements of a [rows, d] input: 37 x 8 = four dense 64-element groups and a ragged one; nl = 5: row-aligned units"""
    g = _gen(f'coupling-{cubic}-{K}-{nl}')
    P = tgs.spline_P(cubic, K)
    table = tgs.put(torch.randn(rows, nl * P, generator=g) * 0.3)
    x32 = torch.randn(rows, d, generator=g) * 1.6                 # ~6 % of the elements in the linear tails
    x = tgs.put(x32.bfloat16() if bf else x32)
    ldj = torch.full((rows,), float('nan'), device=DEV)
    ldiag = torch.full((rows, d), float('nan'), device=DEV)
    with torch.no_grad():
        y = tgs.spline_call(cubic, x, table, nl * P, None, l0, nl, K, reverse, ldj, ldiag)
    return {'y': y, 'ldj': ldj, 'ldiag': ldiag[:, l0:l0 + nl]}


# ---- sx_rqs_inverse_bwd / sx_rqs_forward_bwd / sx_cubic_inverse_bwd / sx_cubic_forward_bwd -------------------------------------------
_OPS = {(False, True): sp.RQSInverse, (False, False): sp.RQSForward, (True, True): sp.CubicInverse, (True, False): sp.CubicForward}


def _element_bwd(cubic, K, reverse, rows=ROWS, d=6, l0=2, nl=2):
    """129 rows x 2 live columns: four 64-element groups and a ragged one over two workgroups; the per-row parameter gradient whole"""
    g = _gen(f'bwd-{cubic}-{K}-{reverse}')
    P = tgs.spline_P(cubic, K)
    params = (torch.randn(rows, nl * P, generator=g) * 0.3).to(DEV).requires_grad_(True)
    x = (torch.randn(rows, d, generator=g) * 1.6).to(DEV).requires_grad_(True)
    gy, gl = torch.randn(rows, d, generator=g).to(DEV), torch.randn(rows, generator=g).to(DEV)
    y, ldj = _OPS[(cubic, reverse)].apply(x, params, None, l0, nl, K, LO, HI, 1.0)
    gx, gp = torch.autograd.grad([y, ldj], [x, params], [gy, gl])
    return {'y': y, 'ldj': ldj, 'gx': gx, 'gparams': gp}


# ---- spline flows of two couplings: the one-launch tier, the slab forward tier, the slab backward ----------------------------------
def _desc(stype, K, hidden, dim=DIM):
    return [{'kind': 'coupling_rqs', 'dim': dim, 'hidden': [hidden], 'n_bins': K, 'lower': LO, 'upper': HI, 'spline_type': stype,
             'mask': 'ordered_right_half' if i % 2 == 0 else 'ordered_left_half', 'latent_dim': 0} for i in range(2)]


def _flow(stype, K, hidden, tag):
    torch.manual_seed(int(_gen(tag).initial_seed()))
    flow = fd.build_flow(st, _desc(stype, K, hidden), DIM)
    with torch.no_grad():
        for p in flow.parameters():
            p.add_(torch.randn_like(p) * 0.05)                    # the last layer's bias starts at zero
    x = torch.randn(ROWS, DIM, generator=_gen(tag + '-x')) * 1.6
    return flow.to(DEV), x.to(DEV)


def _fused(stype, K, precision, hidden=HIDDEN):
    flow, x = _flow(stype, K, hidden, f'flow-{stype}-{K}-{hidden}')
    old = st.set_gemm_precision(precision)
    try:
        with torch.no_grad():
            lp = flow.log_prob(x)
            y, ldj = flow.forward_and_log_det_jacobian(x)
    finally:
        st.set_gemm_precision(old)
    return {'log_prob': lp, 'y': y, 'ldj': ldj}


def _train_step(stype, K=16):
    flow, x = _flow(stype, K, HIDDEN, f'train-{stype}-{K}')
    xg = x.clone().requires_grad_(True)
    wgt = (torch.rand(ROWS, 1, generator=_gen('train-w')) + 0.5).to(DEV)
    lp = flow.log_prob(xg)
    (-(lp * wgt).mean()).backward()
    out = {'log_prob': lp, 'gx': xg.grad}
    out.update({'grad.' + k: p.grad for k, p in flow.named_parameters()})
    return out


# ---- the point-wise kernels whose exp / log are the shared helpers -------------------------------------------------------------------
def _pointwise():
    out = {}
    for kind in (1, 2):                                            # Sigmoid, Logit
        x = tgs.put(tgs.pointwise_input(kind, ROWS, DIM, _gen(f'pw{kind}')))
        y, ldj, ldiag = torch.empty_like(x), torch.full((ROWS,), float('nan'), device=DEV), torch.full((ROWS, DIM), float('nan'), device=DEV)
        with torch.no_grad():
            tgs.pointwise_call(x, kind, 0.0, y, ldj, ldiag)
        out.update({f'{tgs.PW[kind]}.y': y, f'{tgs.PW[kind]}.ldj': ldj, f'{tgs.PW[kind]}.ldiag': ldiag})
    return out


def _pointwise_time():
    g = _gen('pw-time')
    x, t = (torch.randn(ROWS, DIM, generator=g) * 3).to(DEV), (torch.rand(ROWS, 1, generator=g) * 5).to(DEV)
    out = {}
    with torch.no_grad():
        for lt in (False, True):
            f = st.ContinuousTanh(lt)
            y, ld = f.forward_and_log_diag_jacobian(x, t=t)
            xb, ldi = f.inverse_and_log_diag_jacobian(x, t=t)
            out.update({f'tanh{int(lt)}.y': y, f'tanh{int(lt)}.ldiag': ld, f'tanh{int(lt)}.inverse': xb, f'tanh{int(lt)}.inverse_ldiag': ldi})
        out['sigmoid_mix.y'] = st.ContinuousActivation(torch.sigmoid, 2.5).to(DEV)(x, t)
    return out


def _cases():
    c = {}
    for K in (16, 5):                                              # the register path with the LDS-DMA pipeline; the generic branch
        for reverse in (False, True):
            for bf in (False, True):
                c[f'rqs_coupling/K{K}/{"inverse" if reverse else "forward"}/{"bf16" if bf else "f32"}'] = \
                    lambda K=K, reverse=reverse, bf=bf: _coupling(False, K, reverse, bf)
    c['rqs_coupling_row_aligned/K16/inverse/f32'] = lambda: _coupling(False, 16, True, False, nl=5)
    for K in (16, 7):
        for reverse in (False, True):
            c[f'cubic_coupling/K{K}/{"inverse" if reverse else "forward"}'] = lambda K=K, reverse=reverse: _coupling(True, K, reverse, False)
        c[f'cubic_coupling/K{K}/inverse_reference_ldj'] = lambda K=K: _coupling(True, K, 2, False)
    for cubic, Ks in ((False, (16, 5)), (True, (16, 5))):
        for K in Ks:
            for reverse in (True, False):
                c[f'{"cubic" if cubic else "rqs"}_{"inverse" if reverse else "forward"}_bwd/K{K}'] = \
                    lambda cubic=cubic, K=K, reverse=reverse: _element_bwd(cubic, K, reverse)
    for stype, Ks in (('quadratic', (16, 5, 24)), ('cubic', (16, 7))):   # K = 5: the GEN path, K = 24: two tiles per element
        for K in Ks:
            for prec in ('fast', 'exact'):
                c[f'fused/{stype}/K{K}/{prec}'] = lambda stype=stype, K=K, prec=prec: _fused(stype, K, prec)
    for stype in ('quadratic', 'cubic'):
        for K in (16, 7):
            c[f'slab_fwd/{stype}/K{K}'] = lambda stype=stype, K=K: _fused(stype, K, 'fast', hidden=160)
    for stype in ('quadratic', 'cubic'):
        c[f'slab_bwd/{stype}/K16'] = lambda stype=stype: _train_step(stype)
    c['pointwise/sigmoid_logit'] = _pointwise
    c['pointwise_time'] = _pointwise_time
    return c


CASES = _cases()
CU_CASES = ()              # cases whose grid depends on the device's CU count: none at these sizes


def may_be_unstable(case, name):
    """Only the slab backward's parameter gradients (float atomics across workgroups) may be left out of the fixture."""
    return case.startswith('slab_bwd/') and name.startswith('grad.')


def run(name):
    """One case -> {array name: fp32 CPU tensor}."""
    torch.manual_seed(0)
    out = {k: v.detach().float().cpu().contiguous() for k, v in CASES[name]().items()}
    st.check_errors()
    return out


def same_bits(a, b):
    """torch.equal, with NaNs matching NaNs."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def cu_count():
    return torch.cuda.get_device_properties(DEV).multi_processor_count
