"""GPU: the attention core (sx_attention_fwd / sx_attention_bwd, sx_attention.hip) against an independent fp64 oracle, at the
template instantiations and launch shapes test_gpu_attention.py does not reach.

  * the sweep (attncorehelp.CASES): every HALF (4, 8, 16, 32, 64) on both sides of its head-width edge, 1 / 2 / 3 / 4 output tiles
    with the last one full, one column wide and ragged, 1 / 2 / 3 / 4 waves per workgroup with full and one-row last waves, two query
    blocks, and Nq != Nk (the query-owner and the key-owner pass of the backward then pick different wave and block counts).  Four
    sets per case: unmasked, a random {0, 0.5, 1} mask, a structured mask (whole dead tiles first / only the last key live / only
    key 0 live under mask_diagonal) and fully masked.  y, dq, dk and dv, every element, within attncorehelp.bound of the oracle and
    its fp64 autograd: 8 x the error of the fp32 torch composition on the same device tensors, floor 1e-6 * max(1, max |truth|);
  * strides, a batch stride of 0 and 4-byte alignment reproduce the contiguous call bit for bit, forward and backward;
  * logits of 6, 12 and 40 times randn scale, logits shifted by +-300 per query, tile maxima rising at every tile and falling from
    the first, by the same bound (the fp32 composition's own error grows with |logit|, so a fixed tolerance does not serve);
  * the saved log-sum-exp against the oracle's, +inf exactly at the queries without a live key;
  * the C ABI with no key and with no query: y = 0, lse = +inf, dq = 0, dk = dv = 0 out of NaN-filled buffers;
  * launches in which every workgroup of the forward, the query-owner and the key-owner kernel takes a second and a third unit:
    bit for bit the one-unit-per-workgroup launch of the period.

The oracle, the inputs and the conditions on them are checked on the CPU in test_attention_host.py.
"""
import pytest
import torch

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.net.attention import _attention_composed, _core_args

import attncorehelp as ach
import passhelp as ph

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('y', 'dq', 'dk', 'dv')


def _core(q, k, v, gy, H, diag, mask):
    """(y, dq, dk, dv) of st.net.attention and its autograd on device tensors; q, k, v may be views."""
    q, k, v = (t.detach().requires_grad_() if t.is_leaf else t for t in (q, k, v))
    y = st.net.attention(q, k, v, n_heads=H, mask_diagonal=diag, mask=mask)
    return (y.detach(),) + torch.autograd.grad(y, (q, k, v), gy)


def _composed32(q, k, v, gy, H, diag, mask):
    """The fp32 torch composition and its autograd on the same device tensors: the error yardstick."""
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    y = _attention_composed(q, k, v, H, diag, mask)
    return (y.detach(),) + torch.autograd.grad(y, (q, k, v), gy)


def _compare(tag, got, ref, truth):
    """Every element of y, dq, dk, dv within bound(ref32, truth); -> the worst error / bound ratio."""
    worst = 0.0
    for n, g, r in zip(NAMES, got, ref):
        t = truth[n]
        assert g.shape == t.shape and g.dtype == torch.float32, (tag, n)
        assert torch.isfinite(r).all(), (tag, n, 'the fp32 composition is not finite')
        assert not torch.isnan(g).any(), (tag, n)
        tol, e_ref = ach.bound(r.cpu(), t)
        err = (g.cpu().double() - t).abs().max().item()
        print(f'{tag} {n}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e} ratio {err / tol:.3f}')
        assert err <= tol, (tag, n, err, e_ref, tol)
        worst = max(worst, err / tol)
    return worst


def _on_device(c):
    return [c[n].to(DEV) for n in ('q', 'k', 'v', 'gy', 'mask')]


# ---- the sweep --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ach.CASES))
def test_sweep_matches_the_fp64_oracle(name):
    """Forward values and the three gradients of one case in each of its runs (with / without the mask, mask_diagonal where
    Nq == Nk).  Exactly zero: y, dq, dk and dv of the fully masked set, and the y and dq rows of a query whose only live key the
    diagonal removes (query 0 of mask 'c'; by the same construction the last query of mask 'b')."""
    ach.check_conditions(name)
    c = ach.case(name)
    q, k, v, gy, mask = _on_device(c)
    worst = 0.0
    for masked, diag in ach.runs(name):
        mk = mask if masked else None
        got = _core(q, k, v, gy, c['n_heads'], diag, mk)
        ref = _composed32(q, k, v, gy, c['n_heads'], diag, mk)
        worst = max(worst, _compare(f'{name} mask={int(masked)} diag={int(diag)}', got, ref, ach.truth(name, masked, diag)))
        y, dq, dk, dv = got
        if masked:
            for n, t in zip(NAMES, got):
                assert torch.equal(t[3], torch.zeros_like(t[3])), (name, diag, n, 'fully masked set')
        dead = ach.dead_queries(name, masked, diag).to(DEV)
        assert torch.equal(y[dead], torch.zeros_like(y[dead])) and torch.equal(dq[dead], torch.zeros_like(dq[dead]))
        if masked and diag and c['kind'] == 'c':
            assert dead[2, 0] and not dead[2, 1:].any()
    print(f'{name}: worst error / bound {worst:.3f}')


# ---- strides, batch stride 0, alignment ----------------------------------------------------------------------------------------
def _plain(t):
    out = t.detach().clone(memory_format=torch.contiguous_format)
    assert out.is_contiguous() and out.data_ptr() % 16 == 0
    return out


def _same_bits(tag, views, H, diag):
    """st.net.attention on the tensors as they are laid out against the same call on contiguous, 16-byte aligned clones."""
    q, k, v, gy, mask = views
    got = _core(q, k, v, gy, H, diag, mask)
    want = _core(_plain(q), _plain(k), _plain(v), _plain(gy), H, diag, None if mask is None else _plain(mask))
    for n, a, b in zip(NAMES, got, want):
        assert not torch.isnan(b).any() and b.abs().max() > 0, (tag, n)
        assert torch.equal(a, b), (tag, n, (a - b).abs().max().item())


def _draw(tag, *shape):
    return torch.randn(*shape, generator=ph.generator(tag)).to(DEV)


def test_row_strides_reproduce_the_contiguous_bits():
    """q, k and v as column slices of one [R, N, 3 E] buffer (SelfAttention's one-GEMM embedding)."""
    R, N, E, H = 3, 70, 24, 2
    buf = _draw('qkv', R, N, 3 * E).requires_grad_()
    q, k, v = (buf[..., i * E:(i + 1) * E] for i in range(3))
    assert q.stride() == (N * 3 * E, 3 * E, 1)
    mask = ach.random_mask(R, N, ph.generator('qkv mask')).to(DEV)
    gy = _draw('qkv gy', R, N, E)
    _same_bits('slices', (q, k, v, gy, None), H, True)
    _same_bits('slices masked', (q, k, v, gy, mask), H, False)


@pytest.mark.parametrize('Nq,Nk', [(11, 40), (70, 70)])
def test_batch_stride_zero_and_offset_rows_reproduce_the_contiguous_bits(Nq, Nk):
    """q expanded from one set (batch stride 0: InducedSelfAttention's inducing points), k and v rows 3.. of a longer buffer; with
    Nq == Nk under a mask, where the output mask applies."""
    R, E, H = 3, 24, 2
    q = _draw('points', 1, Nq, E).requires_grad_().expand(R, Nq, E)
    k, v = (_draw(n, R, Nk + 3, E).requires_grad_()[:, 3:] for n in ('k rows', 'v rows'))
    assert q.stride(0) == 0 and k.stride(0) == (Nk + 3) * E and not k.is_contiguous()
    mask = ach.random_mask(R, Nk, ph.generator('rows mask')).to(DEV) if Nq == Nk else None
    _same_bits(f'expand {Nq} {Nk}', (q, k, v, _draw('rows gy', R, Nq, E), mask), H, False)


def _offset(t):
    """A copy of `t` that starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def test_four_byte_alignment_reproduces_the_aligned_bits():
    R, N, E, H = 3, 70, 24, 2
    q, k, v, gy = (_offset(_draw(n, R, N, E)).requires_grad_(n != 'gy') for n in ('q', 'k', 'v', 'gy'))
    mask = _offset(ach.random_mask(R, N, ph.generator('offset mask')).to(DEV))
    qv, kv, vv = (t[:] for t in (q, k, v))                      # views of the leaves: the same addresses
    assert all(t.data_ptr() % 16 == 4 for t in (qv, kv, vv, gy, mask))
    _same_bits('offset', (qv, kv, vv, gy, mask), H, True)


# ---- large and shifted logits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(ach.LOGIT_SHAPES))
@pytest.mark.parametrize('variant', ach.LOGIT_VARIANTS)
def test_large_and_shifted_logits(shape, variant):
    """Forward and backward where s * scale is large: the online rescale (rising / falling tile maxima) and the backward's
    P = exp(s * scale - lse) from the saved log-sum-exp, with and without a mask."""
    ach.check_logit_conditions(shape, variant)
    c = ach.logit_case(shape, variant)
    q, k, v, gy, mask = _on_device(c)
    worst = 0.0
    for masked in (False, True):
        mk = mask if masked else None
        got = _core(q, k, v, gy, c['n_heads'], False, mk)
        ref = _composed32(q, k, v, gy, c['n_heads'], False, mk)
        worst = max(worst, _compare(f'{shape} {variant} mask={int(masked)}', got, ref, ach.logit_truth(shape, variant, masked)))
    print(f'{shape} {variant}: worst error / bound {worst:.3f}')


# ---- the saved log-sum-exp -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['a', 'b', 'c'])
def test_log_sum_exp_contract(kind):
    """sx_attention_fwd as AttentionCore.forward calls it: lse is +inf exactly where the oracle's is (set 3; the query whose only
    live key the diagonal removes), and elsewhere within bound of the oracle's, the yardstick being fp32 torch.logsumexp of the
    fp32 logits on the device."""
    R, N, E, H = ach.N_SETS, 70, 24, 2
    g = ph.generator(f'lse {kind}')
    q, k, v = (torch.randn(R, N, E, generator=g) for _ in range(3))
    mask = ach.sets_mask(kind, N, g)
    qd, kd, vd, md = (t.to(DEV) for t in (q, k, v, mask))
    worst = 0.0
    for diag in (False, True):
        y = torch.full((R, N, E), float('nan'), device=DEV)
        lse = torch.full((R, H, N), float('nan'), device=DEV)
        a = _core_args(qd, kd, vd, md.reshape(R, N), H, diag, True)
        _hip.call('sx_attention_fwd', qd, _hip.C.byref(a), y.data_ptr(), lse.data_ptr())
        y64, lse64 = ach.oracle(q, k, v, H, diag, mask)
        inf = torch.isinf(lse64)
        assert inf[3].all() and (lse64[inf] > 0).all() and (diag and kind != 'a') == bool(inf[:3].any())
        assert not torch.isnan(lse).any() and not torch.isnan(y).any()
        assert torch.equal(torch.isinf(lse).cpu() & (lse.cpu() > 0), inf), (kind, diag)
        s = (qd.reshape(R, N, H, E // H).transpose(1, 2) @ kd.reshape(R, N, H, E // H).transpose(1, 2).transpose(-1, -2)) * (H / E) ** 0.5
        s = s.masked_fill((md.reshape(R, 1, 1, N) != 1), -float('inf'))
        if diag:
            s = s.masked_fill(torch.eye(N, dtype=torch.bool, device=DEV), -float('inf'))
        ref = torch.logsumexp(s, -1).cpu()
        tol, e_ref = ach.bound(ref[~inf], lse64[~inf])
        err = (lse.cpu().double()[~inf] - lse64[~inf]).abs().max().item()
        print(f'lse {kind} diag={int(diag)}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e} ratio {err / tol:.3f}')
        assert err <= tol, (kind, diag, err, e_ref, tol)
        worst = max(worst, err / tol)
        tol, _ = ach.bound(_attention_composed(qd, kd, vd, H, diag, md).cpu(), y64)
        assert (y.cpu().double() - y64).abs().max().item() <= tol
    print(f'lse {kind}: worst error / bound {worst:.3f}')


# ---- the empty sides of the C ABI ----------------------------------------------------------------------------------------------
def _abi_args(q, k, v, R, Nq, Nk, E, H):
    a = _hip.sx_attention_args()
    a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    a.q_bs, a.q_rs, a.k_bs, a.k_rs, a.v_bs, a.v_rs = Nq * E, E, Nk * E, E, Nk * E, E
    a.mask, a.mask_bs = None, 0
    a.R, a.Nq, a.Nk, a.E, a.n_heads = R, Nq, Nk, E, H
    a.mask_diagonal, a.out_mask = 0, 0
    return a


def test_c_abi_with_no_key_and_with_no_query():
    """The documented behaviour of the empty sides (stribor_hip.h; "every dq row is written, Nk = 0 included"), which
    AttentionCore never reaches because it answers empty shapes itself.  The empty side is a valid one-element tensor; every output
    starts NaN-filled; the one-element outputs of the empty side are not written."""
    R, N, E, H = 3, 11, 24, 2
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)
    full, gy = _draw('abi full', R, N, E), _draw('abi gy', R, N, E)
    none_k, none_v, none_q, none_y, none_gy, none_lse = (torch.ones(1, device=DEV) for _ in range(6))

    y, lse = nan(R, N, E), nan(R, H, N)
    a = _abi_args(full, none_k, none_v, R, N, 0, E, H)
    _hip.call('sx_attention_fwd', full, _hip.C.byref(a), y.data_ptr(), lse.data_ptr())
    assert torch.equal(y, torch.zeros_like(y))
    assert torch.equal(lse, torch.full_like(lse, float('inf')))

    dq, dk, dv, delta = nan(R, N, E), nan(1), nan(1), nan(R, H, N)
    _hip.call('sx_attention_bwd', full, _hip.C.byref(a), y.data_ptr(), gy.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
              dv.data_ptr(), delta.data_ptr())
    assert torch.equal(dq, torch.zeros_like(dq))
    assert torch.isnan(dk).all() and torch.isnan(dv).all()

    k, v = full, _draw('abi v', R, N, E)
    dq, dk, dv, delta = nan(1), nan(R, N, E), nan(R, N, E), nan(1)
    a = _abi_args(none_q, k, v, R, 0, N, E, H)
    _hip.call('sx_attention_bwd', k, _hip.C.byref(a), none_y.data_ptr(), none_gy.data_ptr(), none_lse.data_ptr(), dq.data_ptr(),
              dk.data_ptr(), dv.data_ptr(), delta.data_ptr())
    assert torch.equal(dk, torch.zeros_like(dk)) and torch.equal(dv, torch.zeros_like(dv))
    assert torch.isnan(dq).all() and torch.isnan(delta).all()


# ---- second and later units per workgroup --------------------------------------------------------------------------------------
PERIOD = 7          # sets: coprime to any grid that is a multiple of the CU count


def _waves(n):
    return min(4, max(1, -(-n // 32)))


def _units_wanted(waves):
    """2.5 x an upper bound of any grid of a kernel with `waves` waves per workgroup: CUs x the workgroups a CU's thread limit
    admits (LDS and registers only lower that)."""
    p = torch.cuda.get_device_properties(DEV)
    cap = p.multi_processor_count * (p.max_threads_per_multi_processor // (64 * waves))
    return 2 * cap + cap // 2


@pytest.mark.parametrize('N,E,H,diag', [(5, 24, 8, False), (130, 16, 1, True), (5, 65, 1, False)],
                         ids=['n5_half4_1wave', 'n130_half8_4waves_2blocks', 'n5_half64'])
def test_second_and_later_units_per_workgroup(N, E, H, diag, request, monkeypatch):
    """All three kernels loop `for (unit = blockIdx.x; unit < n_units; unit += gridDim.x)` with their LDS tiles and per-unit
    registers reused; the grid is capped at CUs x resident workgroups per CU.  A period of 7 distinct sets (set 1 under a
    {0, 0.5, 1} mask, set 2 fully masked) runs on its own, one unit per workgroup, and is held to the oracle; tiled to R sets with
    R * H * blocks >= 2.5 x the largest grid there can be (Nq == Nk: the same count for the key-owner pass), every set of the big
    launch repeats its set of the period bit for bit, forward and backward, out of NaN-filled outputs."""
    ph.poison_outputs(monkeypatch, DEV)
    g = ph.generator(request.node.name)
    q, k, v, gy = (torch.randn(PERIOD, N, E, generator=g) for _ in range(4))
    mask = torch.ones(PERIOD, N, 1)
    mask[1] = ach.random_mask(1, N, g)[0]
    mask[2] = 0
    W = _waves(N)
    blocks = -(-N // (32 * W))
    need = _units_wanted(W)
    R = -(-need // (H * blocks)) + 3
    R += R % PERIOD == 0                                         # (the last pass through the period is cut short)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert R * H * blocks >= need and PERIOD * H * blocks <= cus, (R, H, blocks, need, cus)
    dev = [t.to(DEV) for t in (q, k, v, gy, mask)]
    small = _core(*dev[:4], H, diag, dev[4])
    ref = _composed32(*dev[:4], H, diag, dev[4])
    c = dict(q=q, k=k, v=v, gy=gy, n_heads=H)
    worst = _compare(request.node.name, small, ref, ach.truth_of(c, diag, mask))
    for n, t in zip(NAMES, small):
        assert torch.equal(t[2], torch.zeros_like(t[2])), n
    big = _core(*(ph.tile(t, R) for t in dev[:4]), H, diag, ph.tile(dev[4], R))
    print(f'{request.node.name}: {R} sets, {R * H * blocks} units against 2.5 x cap = {need}; period worst error / bound {worst:.3f}')
    for n, b, s in zip(NAMES, big, small):
        assert b.shape == (R, N, E)
        ph.assert_tiled(f'{request.node.name} {n}', b.reshape(R, N * E), s.reshape(PERIOD, N * E))
