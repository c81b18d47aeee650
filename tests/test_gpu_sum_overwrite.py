"""GPU: the overwrite mode of the fused kernel's batch sum (sx_flow_run3) and the atomic-free empty redo pass.

In overwrite mode the call itself leaves `out` equal to the fp64 batch sum whatever `out` held: the flow kernel's workgroups add their
totals into the library's sum slot (one fp64), the redo pass behind it adds the named samples' rows there and the workgroup that closes
that pass moves the total to `out` and leaves the slot zeroed.
The sums are held to the bound the suite uses elsewhere (tests/test_gpu_base.py): |total - want| <= 1e-9 |want| with
want = log_prob(x).double().sum().  The order of the atomics is not fixed: nothing here compares sums bit for bit.
"""
import ctypes as C
import math

import pytest
import torch

import flowdesc as fd

import stribor_amd as st
from stribor_amd import _hip
from stribor_amd.sharded import ShardedLogProb

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# cfg-2 shape with 2 layers (kernel MODE 5: the fp64 sum lives in LDS), the cfg-4 block once (MODE 7), the cfg-3 shape with 1 layer
# (MODE 3); the workgroup sizes of those kernels (sx_flow_types.h, SX_BLOCK_WAVES) tell that the flow was planned onto them
FLOWS = {'mode5': (lambda: fd.cfg2_desc(2, 64, 64), 64, 512),
         'mode7': (lambda: fd.cfg4_desc(1, 128, 64), 128, 512),
         'mode3': (lambda: fd.cfg3_desc(1, 64, 64, 16), 64, 256)}
POISON = (float('nan'), 7.5)


@pytest.fixture(autouse=True)
def _inference_mode_and_default_precision():
    old = st.set_gemm_precision('fast')
    try:
        with torch.no_grad():
            yield
    finally:
        st.set_gemm_precision(old)
        st.check_errors()


_built = {}


def _flow(which):
    if which not in _built:
        make, dim, block = FLOWS[which]
        torch.manual_seed(3)
        flow = fd.build_flow(st, make(), dim).to(DEV)
        prog = flow._fused_program(True, dim, 0, torch.device(DEV))
        assert prog is not None and prog.launch_info(1 << 24)[1] == block, which
        _built[which] = (flow, prog, dim)
    return _built[which]


def _sizes(prog):
    """(rows per chunk, static row counts, dynamic row counts).  A chunk is one workgroup's rows: 32 per wave (one sample tile per
    wave: SX_NS_FOR = 1), block / 64 waves.  The launcher hands chunks out dynamically when n_chunks > 2 * grid, and its grid is
    min(n_chunks, cap) with cap = the grid of a huge batch: so the smallest dynamic batch is 2 * cap chunks plus ONE row (a last
    chunk of a single row), and (2 * cap + 1) chunks plus 37 rows adds a ragged remainder behind a full last-but-one chunk."""
    cap, block, _ = prog.launch_info(1 << 30)
    rpb = 32 * block // 64
    static = [1, 33, 257, rpb + 1]
    dynamic = [2 * cap * rpb + 1, (2 * cap + 1) * rpb + 37]
    for n in static + dynamic:
        grid = prog.launch_info(n)[0]
        assert (math.ceil(n / rpb) > 2 * grid) == (n in dynamic), (n, grid, rpb)
    return rpb, static, dynamic


def _batch(n, dim, dtype, seed=0):
    x = torch.randn(n, dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    return x.to(dtype)


def _check(total, want, what):
    total, want = total.item(), want.item()
    print(f'{what}: total {total!r} want {want!r} rel {abs(total - want) / abs(want):.3e}')
    assert abs(total - want) <= 1e-9 * abs(want), (what, total, want)


def _redo_head_is_zero():
    torch.cuda.synchronize()
    lists = list(_hip._redo.values())
    assert lists and all(int(t[:2].abs().sum().item()) == 0 for t in lists)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('which', list(FLOWS))
def test_overwrite_ignores_what_out_held(which, dtype):
    """(1) Static and dynamic hand-out, fp32 and bf16 rows, MODE 5 / 7 / 3: `out` pre-filled with NaN and with 7.5 ends up equal to
    the batch sum; the slot is zero again afterwards."""
    flow, prog, dim = _flow(which)
    _, static, dynamic = _sizes(prog)
    big = _batch(max(dynamic), dim, dtype)
    for n in static + dynamic:
        x = big[:n]
        want = flow.log_prob(x).double().sum()
        for fill in POISON:
            out = torch.full((1,), fill, dtype=torch.float64, device=DEV)
            assert flow.log_prob_sum(x, out=out, overwrite=True) is out
            _check(out, want, f'{which} {dtype} n={n} fill={fill}')
        _check(flow.log_prob_sum(x), want, f'{which} {dtype} n={n} out=None')
    torch.cuda.synchronize()
    assert all(float(t.abs().sum().item()) == 0.0 for t in _hip._sum_slots.values())


def test_no_rows_leave_zero():
    """(2) n_rows == 0 in overwrite mode leaves out == 0: through the flow, and through the C entry itself (which returns before any
    kernel launch)."""
    flow, prog, dim = _flow('mode5')
    for fill in POISON:
        out = torch.full((1,), fill, dtype=torch.float64, device=DEV)
        flow.log_prob_sum(torch.empty(0, dim, device=DEV), out=out, overwrite=True)
        assert out.item() == 0.0
        out.fill_(fill)
        x = torch.zeros(1, dim, device=DEV)
        with _hip.device_of(x):
            rc = _hip.lib().sx_flow_run3(C.byref(prog.prog), prog.blobs_for(_hip.GEMM_F16X3).data_ptr(), None, None, x.data_ptr(), None,
                                         _hip.ptr(prog.in_col), _hip.ptr(prog.out_col), None, None, None, out.data_ptr(), None, 0, 0,
                                         None, None, 0, _hip.dtype_code(x), _hip.GEMM_F16X3, _hip.work_counters(x.device).data_ptr(),
                                         _hip.err_flag(x.device), _hip.stream(), _hip.sum_slot(x.device).data_ptr())
        _hip.check(rc, 'sx_flow_run3')
        torch.cuda.synchronize()
        assert out.item() == 0.0


def test_the_slot_rearms_itself():
    """(3) Three calls in a row, static / dynamic / static, each into a differently poisoned buffer: each returns its own sum (a
    slot that kept a total or a count from the call before would show in the next)."""
    flow, prog, dim = _flow('mode5')
    _, static, dynamic = _sizes(prog)
    big = _batch(max(dynamic), dim, torch.float32, seed=1)
    calls = [(static[2], float('nan')), (dynamic[1], 7.5), (static[3], float('inf')), (dynamic[0], -3.0)]
    wants = [flow.log_prob(big[:n]).double().sum() for n, _ in calls]
    outs = [torch.full((1,), fill, dtype=torch.float64, device=DEV) for _, fill in calls]
    for (n, _), out in zip(calls, outs):                     # back to back: no synchronisation between the launches
        flow.log_prob_sum(big[:n], out=out, overwrite=True)
    for (n, fill), out, want in zip(calls, outs, wants):
        _check(out, want, f'call n={n} fill={fill}')


def test_accumulate_is_untouched():
    """(4) A caller's buffer without the keyword is still added to (the old entry's contract: tests/test_gpu_base.py)."""
    for which in FLOWS:
        flow, prog, dim = _flow(which)
        x = _batch(777, dim, torch.float32, seed=2)
        want = flow.log_prob(x).double().sum()
        out = torch.full((1,), 2.5, dtype=torch.float64, device=DEV)
        assert flow.log_prob_sum(x, out=out) is out
        _check(out - 2.5, want, f'{which} accumulate')


@pytest.mark.parametrize('rows', ['one', 'every_group'])
def test_redo_with_overwrite(rows):
    """(5) Rows beyond 2048 are left to the exact pass, which adds them to the main launch's sum before the total goes to `out`.  One such
    row: one listed group, every other workgroup of the redo launch leaves early and must still count itself.  Every 32-row group
    holding one: the whole list.  Static and dynamic batch; the list's head is zero afterwards."""
    flow, prog, dim = _flow('mode5')
    _, static, dynamic = _sizes(prog)
    for n in (8192 + 37, dynamic[1]):
        x = _batch(n, dim, torch.float32, seed=4)
        if rows == 'one':
            x[n // 2, 3] = 5000.0
        else:
            x[::32, 3] = 5000.0
        want = flow.log_prob(x).double().sum()
        assert torch.isfinite(want)
        for fill in POISON:
            out = torch.full((1,), fill, dtype=torch.float64, device=DEV)
            flow.log_prob_sum(x, out=out, overwrite=True)
            _check(out, want, f'redo {rows} n={n} fill={fill}')
            _redo_head_is_zero()
    st.check_errors()


def test_empty_redo_pass_leaves_the_list_alone():
    """(6) An in-range call (empty list: no workgroup of the redo launch counts itself) leaves the list's head zero; a call with named
    rows directly behind it is right (every workgroup counts, the last one out empties the list); an in-range call after that is
    right again."""
    flow, prog, dim = _flow('mode5')
    n = 4096 + 5
    calm = _batch(n, dim, torch.float32, seed=5)
    wild = calm.clone()
    wild[[0, 31, 32, 2000, n - 1], 7] = -4000.0
    want_calm, want_wild = flow.log_prob(calm).double().sum(), flow.log_prob(wild).double().sum()
    assert abs(want_calm.item() - want_wild.item()) > 1e-6 * abs(want_calm.item())
    _check(flow.log_prob_sum(calm), want_calm, 'in range')
    _redo_head_is_zero()
    out_a, out_b, out_c = (torch.full((1,), float('nan'), dtype=torch.float64, device=DEV) for _ in range(3))
    flow.log_prob_sum(calm, out=out_a, overwrite=True)       # back to back
    flow.log_prob_sum(wild, out=out_b, overwrite=True)
    flow.log_prob_sum(calm, out=out_c, overwrite=True)
    _check(out_a, want_calm, 'in range, first')
    _check(out_b, want_wild, 'named rows')
    _check(out_c, want_calm, 'in range, after')
    _redo_head_is_zero()


def test_overwrite_replays_from_a_hip_graph():
    """(7) One overwrite call captured into a HIP graph (single stream) and replayed three times over a re-poisoned `out` and new
    input contents: every replay is right, with no host action between them."""
    flow, prog, dim = _flow('mode5')
    _, static, dynamic = _sizes(prog)
    n = dynamic[1]
    static_x = _batch(n, dim, torch.float32, seed=6)
    static_out = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            flow.log_prob_sum(static_x, out=static_out, overwrite=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        flow.log_prob_sum(static_x, out=static_out, overwrite=True)
    for seed, fill in enumerate((float('nan'), 7.5, float('-inf'))):
        fresh = _batch(n, dim, torch.float32, seed=10 + seed) * (1 + 0.25 * seed)
        static_x.copy_(fresh)
        static_out.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        _check(static_out, flow.log_prob(fresh).double().sum(), f'replay {seed}')


def test_sharded_one_rank():
    """(8) ShardedLogProb on one rank: six asynchronous steps through a ring of four NaN-initialised buffers each give the right sum
    with no zero-fill; a caller-supplied ADDITIVE local_sum still gets a zeroed buffer."""
    flow, prog, dim = _flow('mode5')
    _, static, dynamic = _sizes(prog)
    xs = [_batch(n, dim, torch.bfloat16, seed=20 + i) for i, n in enumerate((dynamic[0], 5000))]
    wants = [flow.log_prob(x).double().sum() for x in xs]
    sh = ShardedLogProb(flow)
    ring = [torch.full((1,), float('nan'), dtype=torch.float64, device=DEV) for _ in range(4)]
    for i in range(6):
        got = sh.log_prob_sum_async(xs[i % 2], ring[i % 4]).wait()
        _check(got, wants[i % 2], f'sharded step {i}')
    _check(sh.log_prob_sum(xs[1]), wants[1], 'sharded log_prob_sum, own buffer')
    additive = ShardedLogProb(local_sum=lambda y, out: flow.log_prob_sum(y, out))
    buf = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV)
    _check(additive.log_prob_sum_async(xs[1], buf).wait(), wants[1], 'additive local_sum, async')
    buf.fill_(7.5)
    _check(additive.log_prob_sum(xs[1], buf), wants[1], 'additive local_sum')


def test_overwrite_without_a_redo_list():
    """A call without a redo pass -- the exact arithmetic, and a launch inside `no_redo` -- has no second launch to hand the sum over:
    the entry clears `out` on the stream instead.  The same contract: NaN and 7.5 are ignored."""
    flow, prog, dim = _flow('mode5')
    _, static, dynamic = _sizes(prog)
    for n in (static[2], dynamic[1]):
        x = _batch(n, dim, torch.float32, seed=7)
        for ctx in ('exact', 'no_redo'):
            st.set_gemm_precision('exact' if ctx == 'exact' else 'fast')
            want = flow.log_prob(x).double().sum()
            for fill in POISON:
                out = torch.full((1,), fill, dtype=torch.float64, device=DEV)
                if ctx == 'no_redo':
                    with _hip.no_redo():
                        flow.log_prob_sum(x, out=out, overwrite=True)
                else:
                    flow.log_prob_sum(x, out=out, overwrite=True)
                _check(out, want, f'{ctx} n={n} fill={fill}')
    st.set_gemm_precision('fast')
