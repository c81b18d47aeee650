"""GPU: how a workgroup of the fused flow kernel loads the rows of a chunk (flow_fused_kernel's chunk loop).

Whole x tiles in identity column order are requested in one flight, and the split-coupling kernels (MODE 5 / 6) on bf16 rows request a
workgroup's NEXT chunk behind the last step of the current one.  None of this changes what is computed, so
  * a row's bits do not depend on which chunk of its workgroup it is in: one call over a batch that gives workgroups a second and a
    third chunk equals, bit for bit, the calls over its 256-row slices -- a slice is a single chunk and takes no early load --, and the
    batch sum equals the fp64 sum of the rows (1e-9 relative: the order of the atomics is free, tests/test_gpu_sum_overwrite.py);
  * at the edges of the early loads -- row counts around a wave's 32, a workgroup's 256 and the launch's first second chunk, on an x
    that ends its allocation and on one that starts inside one -- the rows match the oracle at producthelp.close's tolerance
    (|got - want| <= 1e-5 + 1e-5 |want|, the bound tests/test_gpu_parity.py applies to this flow);
  * a ragged tile (D = 48) and gathered columns (a Flip), which keep the old loads, still match the oracle;
  * a row of |x| ~ 3000 in a second-pass chunk is redone by the exact kernel (bit for bit what 'exact' gives) and leaves its
    neighbours' bits alone;
  * cfg 3 and cfg 4, which share the loop, match the oracle over second-pass row counts of their own.
"""
import os
import sys

import pytest
import torch

import flowdesc as fd
from producthelp import close

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import stribor_oracle as orc

import stribor_amd as st

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def _inference_mode_and_default_precision():
    old = st.set_gemm_precision('fast')
    try:
        with torch.no_grad():
            yield
    finally:
        st.set_gemm_precision(old)
        st.check_errors()


def _cap_and_rows_per_chunk(flow, dim):
    prog = flow._fused_program(True, dim, 0, torch.device(DEV))
    assert prog is not None
    cap, block, _ = prog.launch_info(1 << 30)
    return cap, 32 * block // 64


_flows = {}


def _cfg2(layers):
    """One cfg 2 flow per depth (D 64, hidden 64), its oracle spec, the launch's workgroup cap."""
    if layers not in _flows:
        torch.manual_seed(23 + layers)
        desc = fd.cfg2_desc(layers, 64, 64)
        flow = fd.build_flow(st, desc, 64)
        spec = fd.flow_spec(desc, {k: v.clone() for k, v in flow.state_dict().items()})
        flow = flow.to(DEV)
        cap, rpb = _cap_and_rows_per_chunk(flow, 64)
        assert rpb == 256, rpb
        _flows[layers] = (flow, spec, cap)
    return _flows[layers]


# ---- 1. a row's bits do not depend on its chunk ------------------------------------------------------------------------------------
_sliced = {}


def _sliced_case(layers, storage):
    """The longest batch of the case, once: the flow, x, and per direction the results of its 256-row slices (the shorter batch is a
    prefix: whole slices are shared, only its ragged last slice is evaluated again)."""
    key = (layers, storage)
    if key not in _sliced:
        flow, _, cap = _cfg2(layers)
        n = 3 * cap * 256 + 1
        x = torch.randn(n, 64, generator=torch.Generator().manual_seed(7), dtype=torch.float32).to(DEV)
        x = x.bfloat16() if storage == 'bf16' else x
        lp, y = [], []
        for a in range(0, n, 256):
            lp.append(flow.log_prob(x[a:a + 256]))
            y.append(flow.forward(x[a:a + 256]))
        _sliced[key] = (flow, cap, x, lp, y)
    return _sliced[key]


@pytest.mark.parametrize('passes', [2, 3], ids=['second_chunk', 'third_chunk'])
@pytest.mark.parametrize('storage', ['bf16', 'f32'])
@pytest.mark.parametrize('layers', [1, 8])
def test_a_rows_bits_do_not_depend_on_its_chunk(layers, storage, passes):
    flow, cap, x, lp_slices, y_slices = _sliced_case(layers, storage)
    n = cap * 256 + 37 if passes == 2 else 3 * cap * 256 + 1
    assert flow._fused_program(True, 64, 0, torch.device(DEV)).launch_info(n)[0] * 256 * (passes - 1) < n
    whole, last = n // 256, n % 256
    xs = x[:n]
    want_lp = torch.cat(lp_slices[:whole] + [flow.log_prob(xs[whole * 256:])])
    want_y = torch.cat(y_slices[:whole] + [flow.forward(xs[whole * 256:])])
    assert last and want_lp.shape == (n, 1) and want_y.shape == (n, 64)
    got_lp = flow.log_prob(xs)
    differ = int((got_lp != want_lp).sum())
    print(f'layers {layers} {storage} n {n}: log_prob rows that differ from their slice: {differ}')
    assert torch.equal(got_lp, want_lp)
    got_y = flow.forward(xs)
    assert got_y.dtype == want_y.dtype
    differ = int((got_y != want_y).any(-1).sum())
    print(f'layers {layers} {storage} n {n}: forward rows that differ from their slice: {differ}')
    assert torch.equal(got_y, want_y)
    total, rows = flow.log_prob_sum(xs).item(), got_lp.double().sum().item()
    print(f'layers {layers} {storage} n {n}: sum {total!r} rows {rows!r}')
    assert abs(total - rows) <= 1e-9 * abs(rows), (total, rows)


# ---- 2. edges of the early loads ----------------------------------------------------------------------------------------------------
_edge = {}


def _edge_case(storage):
    """One allocation of cap * 256 + 1 + 5 rows and the oracle's log_prob / forward of every row of it."""
    if storage not in _edge:
        flow, spec, cap = _cfg2(2)
        big = torch.randn(cap * 256 + 6, 64, generator=torch.Generator().manual_seed(9))
        big = big.bfloat16() if storage == 'bf16' else big
        seen = big.float()                               # the values the kernel reads
        _edge[storage] = (flow, cap, big.to(DEV), orc.flow_log_prob(spec, seen), orc.flow_forward_and_ldj(spec, seen))
    return _edge[storage]


@pytest.mark.parametrize('where', ['end_of_allocation', 'row_offset'])
@pytest.mark.parametrize('storage', ['bf16', 'f32'])
def test_edges_of_the_early_loads(storage, where):
    flow, cap, big, want_lp, (want_y, want_ldj) = _edge_case(storage)
    total = big.shape[0]
    for n in (1, 31, 33, 255, 257, cap * 256 - 1, cap * 256, cap * 256 + 1):
        a = total - n if where == 'end_of_allocation' else 5         # the view's last row is the allocation's last / its first is row 5
        x = big[a:a + n]
        assert x.is_contiguous() and x.storage_offset() == a * 64
        got = flow.log_prob(x)
        assert got.shape == (n, 1)
        close(got, want_lp[a:a + n])
        if storage == 'f32':                                         # (a bf16 y is a rounded store: tests/test_gpu_storage.py)
            y, ldj = flow.forward_and_log_det_jacobian(x)
            close(y, want_y[a:a + n])
            close(ldj, want_ldj[a:a + n], atol=1e-4)


# ---- 3. shapes that stay on the old loads -------------------------------------------------------------------------------------------
def _ragged_desc():
    return fd.cfg2_desc(2, 48, 64), 48


def _flip_desc():
    d = fd.cfg2_desc(2, 64, 64)
    return [d[0], {'kind': 'flip'}, d[1]], 64


@pytest.mark.parametrize('make', [_ragged_desc, _flip_desc], ids=['ragged_tile_d48', 'flip_gathered_columns'])
@pytest.mark.parametrize('storage', ['bf16', 'f32'])
def test_shapes_that_stay_on_the_old_loads(make, storage):
    torch.manual_seed(3)
    desc, dim = make()
    flow = fd.build_flow(st, desc, dim)
    spec = fd.flow_spec(desc, {k: v.clone() for k, v in flow.state_dict().items()})
    flow = flow.to(DEV)
    assert flow._fused_program(True, dim, 0, torch.device(DEV)) is not None
    x = torch.randn(257, dim)
    x = x.bfloat16() if storage == 'bf16' else x
    close(flow.log_prob(x.to(DEV)), orc.flow_log_prob(spec, x.float()))
    if storage == 'f32':
        y, ldj = flow.forward_and_log_det_jacobian(x.to(DEV))
        wy, wl = orc.flow_forward_and_ldj(spec, x)
        close(y, wy)
        close(ldj, wl, atol=1e-4)


# ---- 4. the redo pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage', ['bf16', 'f32'])
def test_a_wild_row_in_a_second_pass_chunk_is_redone(storage):
    flow, _, cap = _cfg2(2)
    n = cap * 256 + 37
    at = cap * 256 + 17                                  # chunk `cap`: some workgroup's second
    calm = torch.randn(n, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    wild = calm.clone()
    wild[at] *= 3000.0 / wild[at].abs().max()
    if storage == 'bf16':
        calm, wild = calm.bfloat16(), wild.bfloat16()
    keep = torch.arange(n, device=DEV) != at
    base = flow.log_prob(calm)
    got = flow.log_prob(wild)
    st.check_errors()
    st.set_gemm_precision('exact')
    exact = flow.log_prob(wild)
    st.set_gemm_precision('fast')
    assert torch.isfinite(got).all()
    assert torch.equal(got[at], exact[at]), (got[at].item(), exact[at].item())
    assert torch.equal(got[keep], base[keep])


# ---- 5. the other fused configurations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cfg3', 'cfg4'])
def test_other_fused_configurations_over_a_second_pass(name):
    """Rows are independent, so the oracle evaluates the rows that matter: the first chunk's and everything from the last first-pass
    chunk's tail on -- chunks `cap` and beyond are somebody's second.  Every row enters the batch sum."""
    torch.manual_seed(6)
    desc, dim = (fd.cfg3_desc(2, 64, 64), 64) if name == 'cfg3' else (fd.cfg4_desc(1, 128, 64), 128)      # (cfg 4: one block, two couplings)
    flow = fd.build_flow(st, desc, dim)
    spec = fd.flow_spec(desc, {k: v.clone() for k, v in flow.state_dict().items()})
    flow = flow.to(DEV)
    cap, rpb = _cap_and_rows_per_chunk(flow, dim)
    n = cap * rpb + 37
    assert flow._fused_program(True, dim, 0, torch.device(DEV)).launch_info(n)[0] * rpb < n
    x = torch.randn(n, dim, generator=torch.Generator().manual_seed(8))
    if name == 'cfg3':
        x = x.clamp(-2.9, 2.9)                           # inside the splines' interval
    got = flow.log_prob(x.to(DEV))
    assert got.shape == (n, 1) and torch.isfinite(got).all()
    for rows in (slice(0, rpb), slice(cap * rpb - 33, n)):
        close(got[rows], orc.flow_log_prob(spec, x[rows]))
    total, rows = flow.log_prob_sum(x.to(DEV)).item(), got.double().sum().item()
    print(f'{name} n {n}: sum {total!r} rows {rows!r}')
    assert abs(total - rows) <= 1e-9 * abs(rows), (total, rows)
