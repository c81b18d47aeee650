"""GPU: the k16-step-grain schedule of the split-coupling step on 1 + 1 tiles, hidden 33..64 (coupling_affine_ks, kernel MODE 5 / 6).

The schedule re-orders the step's instructions and changes none of them, so
  * on fixture F4's flow every row comes out with the bits the parent build produced (tests/golden/f23_cfg2_parent_bits.npz, written by
    tools/make_parent_bits.py against the parent's library: outputs only; F4 holds 256 rows, all of them are stored);
  * at the seams of the launch (rows around a wave's 32 and a workgroup's 256, a batch that gives some workgroup a second chunk) both
    directions match the oracle at the tolerance tests/test_gpu_parity.py applies to F4 (|got - want| <= 1e-5 + 1e-5 |want|) and the
    batch sum equals the fp64 sum of the rows (1e-9 relative: the order of the atomics is free, tests/test_gpu_sum_overwrite.py);
  * hidden 32 and D = 128 -- shapes that stay on the old step -- still match the oracle;
  * a row of |x| ~ 3000 is named, redone by the exact kernel (bit for bit what 'exact' gives), and leaves its neighbours' bits alone.
"""
import os
import sys

import numpy as np
import pytest
import torch

import flowdesc as fd
from goldens import GOLDEN_DIR, Golden
from producthelp import close, product_flow

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import stribor_oracle as orc

import stribor_amd as st

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEAM_ROWS = (1, 31, 32, 33, 255, 256, 257)


@pytest.fixture(autouse=True)
def _inference_mode_and_default_precision():
    old = st.set_gemm_precision('fast')
    try:
        with torch.no_grad():
            yield
    finally:
        st.set_gemm_precision(old)
        st.check_errors()


@pytest.mark.parametrize('storage', ['f32', 'bf16'])
def test_rows_keep_the_parents_bits(storage):
    g = Golden('f4_cfg2')
    want = np.load(os.path.join(GOLDEN_DIR, 'f23_cfg2_parent_bits.npz'))
    flow = product_flow(g, 'cfg2')
    x = g.t('cfg2/x').to(DEV)
    x = x.bfloat16() if storage == 'bf16' else x
    for name, got in (('log_prob', flow.log_prob(x)), ('forward', flow.forward(x)[:257]), ('inverse', flow.inverse(x)[:257])):
        ref = torch.from_numpy(want[f'{storage}/{name}'])
        got = got.float().cpu()
        diff = (got != ref) & ~(got.isnan() & ref.isnan())
        print(f'{storage}/{name}: {int(diff.sum())} of {ref.numel()} values differ from the parent build')
        assert got.shape == ref.shape and torch.equal(got, ref), (storage, name)


_seam = {}


def _seam_case(layers):
    """One flow per depth, one batch and one oracle evaluation (both directions) shared by every row count."""
    if layers not in _seam:
        torch.manual_seed(11 + layers)
        desc = fd.cfg2_desc(layers, 64, 64)
        flow = fd.build_flow(st, desc, 64)
        spec = fd.flow_spec(desc, {k: v.clone() for k, v in flow.state_dict().items()})
        flow = flow.to(DEV)
        prog = flow._fused_program(True, 64, 0, torch.device(DEV))
        assert prog is not None
        cap, block, _ = prog.launch_info(1 << 30)
        rpb = 32 * block // 64
        assert rpb == 256, block
        second = cap * rpb + 37                      # one chunk more than workgroups: somebody takes a second one
        assert prog.launch_info(second)[0] * rpb < second
        x = torch.randn(second, 64, generator=torch.Generator().manual_seed(5))
        _seam[layers] = (flow, x.to(DEV), orc.flow_log_prob(spec, x), orc.flow_forward_and_ldj(spec, x), second)
    return _seam[layers]


@pytest.mark.parametrize('direction', ['log_prob', 'forward'])
@pytest.mark.parametrize('layers', [1, 2, 8])
def test_seams_against_the_oracle(layers, direction):
    flow, x, want_lp, (want_y, want_ldj), second = _seam_case(layers)
    for n in SEAM_ROWS + (second,):
        if direction == 'log_prob':                  # the inverse direction: MODE 5
            got = flow.log_prob(x[:n])
            assert got.shape == (n, 1)
            close(got, want_lp[:n])
            total, rows = flow.log_prob_sum(x[:n]).item(), got.double().sum().item()
            print(f'layers {layers} n {n}: sum {total!r} rows {rows!r}')
            assert abs(total - rows) <= 1e-9 * abs(rows), (layers, n, total, rows)
        else:                                        # MODE 6
            y, ldj = flow.forward_and_log_det_jacobian(x[:n])
            close(y, want_y[:n])
            close(ldj, want_ldj[:n], atol=1e-4)


@pytest.mark.parametrize('dim,hidden', [(64, 32), (128, 64)], ids=['hidden32', 'dim128'])
def test_other_shapes_stay_on_the_old_step(dim, hidden):
    torch.manual_seed(2)
    desc = fd.cfg2_desc(2, dim, hidden)
    flow = fd.build_flow(st, desc, dim)
    spec = fd.flow_spec(desc, {k: v.clone() for k, v in flow.state_dict().items()})
    flow = flow.to(DEV)
    x = torch.randn(257, dim)
    close(flow.log_prob(x.to(DEV)), orc.flow_log_prob(spec, x))
    y, ldj = flow.forward_and_log_det_jacobian(x.to(DEV))
    wy, wl = orc.flow_forward_and_ldj(spec, x)
    close(y, wy)
    close(ldj, wl, atol=1e-4)


def test_a_row_out_of_range_is_named_and_redone():
    torch.manual_seed(4)
    flow = fd.build_flow(st, fd.cfg2_desc(2, 64, 64), 64).to(DEV)
    calm = torch.randn(33, 64, device=DEV)
    wild = calm.clone()
    wild[17] *= 3000.0 / wild[17].abs().max()
    keep = torch.arange(33, device=DEV) != 17
    base = flow.log_prob(calm)
    got = flow.log_prob(wild)
    st.check_errors()
    st.set_gemm_precision('exact')
    exact = flow.log_prob(wild)
    st.set_gemm_precision('fast')
    assert torch.isfinite(got).all()
    assert torch.equal(got[17], exact[17]), (got[17].item(), exact[17].item())
    assert torch.equal(got[keep], base[keep])
