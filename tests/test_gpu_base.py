"""GPU: the base densities Normal / MultivariateNormal / Uniform -- sx_base_logprob, sx_normal_logprob_bwd, sx_mvn_logprob
(csrc/sx_base.hip), the classes over them, and NormalizingFlow.log_prob / log_prob_sum with such a base (one launch or two).

Truth: torch.distributions in fp64 on the CPU.  Reference error e_ref: torch.distributions in fp32 on the device.  Bound:
cnfhelp.bound, 8 x e_ref floored at 1e-6 * max(1, max |truth|).  Rows outside a Uniform's support are -inf on both sides and are
compared as such; the bound applies to the finite rows."""
import copy

import pytest
import torch

import basehelp as bh
import cnfhelp as ch
import passhelp as ph
from storagehelp import bits, offset_view

import stribor_amd as st
from oracle import stribor_oracle as orc
from stribor_amd import _hip
from stribor_amd.util import flowdesc as fd

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROWS = (1, 33, 130)


def held(tag, got, ref32, truth64):
    """got (device fp32) against truth64 (CPU fp64) within cnfhelp.bound(ref32, truth64) on the finite entries; the others equal."""
    got, ref32, truth64 = got.detach().cpu().double(), ref32.detach().cpu(), truth64.detach().cpu()
    assert got.shape == truth64.shape == ref32.shape, (tag, got.shape, ref32.shape, truth64.shape)
    fin = torch.isfinite(truth64)
    assert torch.equal(got[~fin].nan_to_num(nan=12345.0), truth64[~fin].nan_to_num(nan=12345.0)), tag
    if not fin.any():
        return
    tol, e_ref = ch.bound(ref32[fin], truth64[fin])
    err = (got[fin] - truth64[fin]).abs().max().item()
    print(f'{tag}: err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e}')
    assert err <= tol, (tag, err, e_ref, tol)


def truth_and_ref(d, x, ldj=None):
    """(fp64 CPU truth, fp32 device reference) of d.log_prob(x) (+ ldj); x as the kernel sees it (bf16 rows: their fp32 values)."""
    xf = x.detach().float()
    t = bh.torch_dist(d, torch.float64, 'cpu').log_prob(xf.cpu().double())
    r = bh.torch_dist(d, torch.float32, DEV).log_prob(xf.to(DEV))
    if ldj is not None:
        t, r = t + ldj.detach().cpu().double().reshape(t.shape), r + ldj.detach().to(DEV).reshape(r.shape)
    return t, r


def make_dist(kind, D, gen):
    if kind == 'normal':
        return st.Normal(torch.randn(D, generator=gen), 0.5 + 1.5 * torch.rand(D, generator=gen))
    if kind == 'uniform':
        low = torch.randn(D, generator=gen) - 3.0
        return st.Uniform(low, low + 6.0 + torch.rand(D, generator=gen))
    return st.MultivariateNormal(torch.randn(D, generator=gen), scale_tril=bh.well_conditioned_tril(D, gen))


def draw(d, n, D, gen):
    """Rows inside the support of d (CPU fp32)."""
    if isinstance(d, st.Uniform):                    # (a margin of 1 % of the width: bf16 storage keeps every row inside)
        return d.low + (0.01 + 0.98 * torch.rand(n, D, generator=gen)) * (d.high - d.low)
    return torch.randn(n, D, generator=gen) * 1.5


# ---- the kernels' values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('kind,D', [(k, D) for k in ('normal', 'uniform') for D in (1, 3, 5, 32, 33, 64, 128)]
                         + [('mvn', D) for D in (1, 3, 32, 33, 64, 96, 128)])
def test_kernel_values(kind, D, dtype, monkeypatch):
    """Rows 1 / 33 / 130, with and without the log-det, aligned and one element past a 16-byte boundary, and a [2, 3, D] batch through
    the public log_prob; outputs start as NaN."""
    ph.poison_outputs(monkeypatch, DEV)
    gen = ph.generator(f'values/{kind}/{D}')
    d_cpu = make_dist(kind, D, gen)
    d = copy.deepcopy(d_cpu).to(DEV)
    for n in ROWS:
        x = draw(d_cpu, n, D, gen).to(dtype)
        ldj = torch.randn(n, generator=gen)
        for off in (0, 1):
            xd = offset_view(x.to(DEV), off)
            for l in (None, ldj):
                got = d._kernel_rows(xd, None if l is None else l.to(DEV))
                assert got is not None and got.dtype == torch.float32 and got.shape == (n,)
                t, r = truth_and_ref(d_cpu, x, l)
                held(f'{kind} D={D} n={n} off={off} ldj={l is not None}', got, r, t)
    x3 = draw(d_cpu, 6, D, gen).reshape(2, 3, D).to(dtype)
    got = d.log_prob(x3.to(DEV))
    t, r = truth_and_ref(d_cpu, x3)
    assert got.shape == (2, 3)
    held(f'{kind} D={D} [2, 3, D]', got, r, t)


@pytest.mark.parametrize('kind,D,dtype', [('normal', 8, torch.float32), ('uniform', 5, torch.float32), ('normal', 16, torch.bfloat16),
                                          ('mvn', 33, torch.float32)])
def test_second_trip_of_a_capped_grid(kind, D, dtype, monkeypatch):
    """The launchers cap their grids (2048 workgroups; the multivariate normal at the resident workgroups): a batch of 2.5 x the
    largest possible grid in 128-row passes gives every wave a second trip.  Its rows repeat a 77-row period and must equal the
    period's own result bit for bit."""
    ph.poison_outputs(monkeypatch, DEV)
    gen = ph.generator(f'trip/{kind}/{D}')
    d_cpu = make_dist(kind, D, gen)
    d = copy.deepcopy(d_cpu).to(DEV)
    n = ph.big_rows(DEV)
    ph.assert_multi_pass(n, 1, DEV)
    assert n >= 2.5 * 2048 * 256 / 2                 # (sx_base_logprob: at least 2 rows' lanes per row here, 2048 blocks of 256 at the most)
    small = draw(d_cpu, ph.ROW_PERIOD, D, gen).to(dtype).to(DEV)
    l_small = torch.randn(ph.ROW_PERIOD, generator=gen).to(DEV)
    want = d._kernel_rows(small, l_small)
    t, r = truth_and_ref(d_cpu, small.cpu(), l_small.cpu())
    held(f'period {kind} D={D}', want, r, t)
    got = d._kernel_rows(ph.tile(small, n), ph.tile(l_small, n))
    ph.assert_tiled(f'{kind} D={D}', got.unsqueeze(-1), want.unsqueeze(-1))


def test_uniform_edges_and_nan_rows(monkeypatch):
    """x == low is inside, x == high outside; one element outside makes exactly its row -inf; a NaN stays in its row -- for the three
    kernels, on both layouts of sx_base_logprob (vector: D = 8; one wave per row: D = 5) and on one and two tiles of sx_mvn_logprob."""
    ph.poison_outputs(monkeypatch, DEV)
    gen = ph.generator('edges')
    for D in (5, 8, 64):
        low = (torch.randn(D, generator=gen) - 3.0).bfloat16().float()              # bounds that bf16 holds exactly: x == low and
        high = (low + 6.0 + torch.rand(D, generator=gen)).bfloat16().float()        # x == high survive the storage
        u_cpu = st.Uniform(low, high)
        u = copy.deepcopy(u_cpu).to(DEV)
        log_norm = -(high.double() - low.double()).log().sum().item()
        for dtype in (torch.float32, torch.bfloat16):
            x = draw(u_cpu, 40, D, gen)
            x[3, D - 1] = low[D - 1]                 # on the lower bound: inside
            x[7, 0] = high[0]                        # on the upper bound: outside
            x[11, D // 2] = high[D // 2] + 1.0
            x[12, 1] = low[1] - 0.5
            if dtype == torch.float32:               # the next fp32 below the lower bound, and the last one below the upper bound
                x[13, 2] = torch.nextafter(low[2], torch.tensor(-float('inf')))
                x[14, 2] = torch.nextafter(high[2], torch.tensor(-float('inf')))
            else:
                x[13, 2] = low[2] - 0.5
            x[20, D - 2] = float('nan')
            x[21, 0], x[21, 1] = float('nan'), high[1] + 1.0                         # NaN and outside in one row: NaN
            got = u.log_prob(x.to(dtype).to(DEV)).cpu()
            inf_rows, nan_rows = [7, 11, 12, 13], [20, 21]
            assert torch.isinf(got[inf_rows]).all() and (got[inf_rows] < 0).all(), (D, dtype, got[inf_rows])
            assert torch.isnan(got[nan_rows]).all(), (D, dtype, got[nan_rows])
            rest = [i for i in range(40) if i not in inf_rows + nan_rows]
            assert torch.equal(got[rest], torch.full((len(rest),), log_norm, dtype=torch.float64).float()), (D, dtype, got)
    for kind, D in (('normal', 5), ('normal', 8), ('mvn', 5), ('mvn', 40)):
        d_cpu = make_dist(kind, D, gen)
        d = copy.deepcopy(d_cpu).to(DEV)
        x = draw(d_cpu, 70, D, gen)
        x[0, 0] = x[33, D - 1] = x[69, D // 2] = float('nan')
        got = d.log_prob(x.to(DEV)).cpu()
        nan_rows = [0, 33, 69]
        assert torch.isnan(got[nan_rows]).all()
        rest = [i for i in range(70) if i not in nan_rows]
        t, r = truth_and_ref(d_cpu, x[rest])
        held(f'NaN rows {kind} D={D}', got[rest], r, t)


@pytest.mark.parametrize('case', sorted(bh.f21_cases()))
def test_f21_cases(case):
    make, x, lp32, lp64, _ = bh.f21_cases()[case]
    got = make().to(DEV).log_prob(x.to(DEV))
    held(f'F21 {case}', got, lp32, lp64)


def test_out_of_coverage_routes():
    """Batch-shaped parameters, the float form and a 129-column multivariate normal are evaluated as torch ops on the device: the same
    values within the bound."""
    gen = ph.generator('coverage')
    x = torch.randn(6, 5, generator=gen)
    b_cpu = st.Normal(torch.randn(4, 1, 5, generator=gen), 0.5 + torch.rand(5, generator=gen))
    assert copy.deepcopy(b_cpu).to(DEV)._kernel_rows(x.to(DEV), None) is None
    got = copy.deepcopy(b_cpu).to(DEV).log_prob(x.to(DEV))
    t, r = truth_and_ref(b_cpu, x)
    assert got.shape == (4, 6)
    held('batch-shaped Normal', got, r, t)
    ub_cpu = st.Uniform(torch.zeros(2, 1, 5) - 4.0, torch.full((5,), 4.0))
    got = copy.deepcopy(ub_cpu).to(DEV).log_prob(x.to(DEV))
    t, r = truth_and_ref(ub_cpu, x)
    held('batch-shaped Uniform', got, r, t)
    for f_cpu in (st.Normal(0.5, 2.0), st.Uniform(-8.0, 8.0)):
        got = copy.deepcopy(f_cpu).to(DEV).log_prob(x.to(DEV))
        t, r = truth_and_ref(f_cpu, x)
        assert got.shape == (6, 5)
        held(f'float form {type(f_cpu).__name__}', got, r, t)
    m_cpu = make_dist('mvn', 129, gen)
    xm = torch.randn(33, 129, generator=gen)
    m = copy.deepcopy(m_cpu).to(DEV)
    assert m._kernel_rows(xm.to(DEV), None) is None
    t, r = truth_and_ref(m_cpu, xm)
    held('MVN D=129', m.log_prob(xm.to(DEV)), r, t)
    mb_cpu = st.MultivariateNormal(torch.randn(3, 4, generator=gen), scale_tril=bh.well_conditioned_tril(4, gen))
    x4 = torch.randn(7, 1, 4, generator=gen)
    t, r = truth_and_ref(mb_cpu, x4)
    held('batch-shaped MVN', copy.deepcopy(mb_cpu).to(DEV).log_prob(x4.to(DEV)), r, t)


# ---- backward ----------------------------------------------------------------------------------------------------------------------
def torch_grads(make, tensors, x, w, dtype, device):
    """Gradients of sum(w * log_prob(x)) by torch autograd: make(*leaves) -> torch distribution.  -> [gx, *g_params]"""
    leaves = [t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in tensors]
    xl = x.detach().to(device=device, dtype=dtype).requires_grad_(True)
    (make(*leaves).log_prob(xl) * w.to(device=device, dtype=dtype)).sum().backward()
    return [xl.grad] + [l.grad for l in leaves]


@pytest.mark.parametrize('D', [3, 32, 33, 128])
@pytest.mark.parametrize('n', ROWS)
def test_normal_backward(n, D):
    """dx, d loc, d scale of sx_normal_logprob_bwd against fp64 autograd; e_ref: fp32 torch autograd on the device.  Two backward
    calls return the same bits."""
    import torch.distributions as td
    gen = ph.generator(f'bwd/{n}/{D}')
    loc, scale = torch.randn(D, generator=gen), 0.5 + 1.5 * torch.rand(D, generator=gen)
    x, w = torch.randn(n, D, generator=gen) * 1.5, torch.randn(n, generator=gen)
    make = lambda l, s: td.Independent(td.Normal(l, s, validate_args=False), 1)
    truth = torch_grads(make, (loc, scale), x, w, torch.float64, 'cpu')
    ref = torch_grads(make, (loc, scale), x, w, torch.float32, DEV)
    runs = []
    for _ in range(2):
        d = st.Normal(torch.nn.Parameter(loc.clone()), torch.nn.Parameter(scale.clone())).to(DEV)
        xd = x.to(DEV).requires_grad_(True)
        lp = d.log_prob(xd)
        assert lp.requires_grad and lp.shape == (n,)
        (lp * w.to(DEV)).sum().backward()
        runs.append([xd.grad, d.loc.grad, d.scale.grad])
    for name, g, r, t in zip(('gx', 'g_loc', 'g_scale'), runs[0], ref, truth):
        held(f'Normal bwd n={n} D={D} {name}', g, r, t)
    for a, b in zip(*runs):
        assert torch.equal(bits(a), bits(b))
    t, r = truth_and_ref(st.Normal(loc, scale), x)
    held(f'Normal fwd (graph) n={n} D={D}', lp, r, t)


@pytest.mark.parametrize('n,D', [(100003, 3), (20483, 33), (20483, 128)])
def test_normal_backward_beyond_the_block_cap(n, D):
    """sx_normal_logprob_bwd caps its grid (1024 blocks): beyond 1024 x row lanes rows a thread owns several rows of its block's
    slab -- here slabs of 2 x 64 rows (D = 3: 64 row lanes) and of 6 x 4 rows (D = 33, 128: 4 row lanes), with a ragged last block.
    dx equals, bit for bit, the same rows run in small batches (one row per thread); d loc / d scale are held to fp64 autograd
    (e_ref: fp32 torch autograd on the device); two calls return the same bits."""
    import torch.distributions as td
    gen = ph.generator(f'bwd-cap/{n}/{D}')
    loc, scale = torch.randn(D, generator=gen), 0.5 + 1.5 * torch.rand(D, generator=gen)
    x, w = torch.randn(n, D, generator=gen) * 1.5, torch.randn(n, generator=gen) / n ** 0.5
    blocks = _hip.lib().sx_normal_bwd_partial_floats(n, D) // (2 * D)
    row_lanes = 256 // min(64, 1 << (D - 1).bit_length())
    slab = -(-n // blocks)
    assert blocks <= 1024 and slab >= 2 * row_lanes and n % slab != 0, (blocks, row_lanes, slab)      # several trips, ragged end
    make = lambda l, s: td.Independent(td.Normal(l, s, validate_args=False), 1)
    truth = torch_grads(make, (loc, scale), x, w, torch.float64, 'cpu')
    ref = torch_grads(make, (loc, scale), x, w, torch.float32, DEV)

    def run(xs, ws):
        d = st.Normal(torch.nn.Parameter(loc.clone()), torch.nn.Parameter(scale.clone())).to(DEV)
        xd = xs.to(DEV).requires_grad_(True)
        (d.log_prob(xd) * ws.to(DEV)).sum().backward()
        return xd.grad, d.loc.grad, d.scale.grad
    first, second = run(x, w), run(x, w)
    for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b))
    for name, g, r, t in zip(('gx', 'g_loc', 'g_scale'), first, ref, truth):
        held(f'Normal bwd beyond the cap n={n} D={D} {name}', g, r, t)
    for lo in (0, max(slab - 65, 7), n - 130):               # the first rows, rows across a slab boundary, the ragged last block
        small = run(x[lo:lo + 130], w[lo:lo + 130])[0]
        assert torch.equal(bits(first[0][lo:lo + 130]), bits(small)), lo


def test_uniform_backward_and_scalar_parameters():
    import torch.distributions as td
    gen = ph.generator('bwd/uniform')
    n, D = 33, 5
    low = torch.randn(D, generator=gen) - 3.0
    high = low + 6.0 + torch.rand(D, generator=gen)
    x = low + torch.rand(n, D, generator=gen) * (high - low) * 0.99
    x[4, 2] = high[2] + 1.0                          # a row outside the support: the bounds' gradients do not see it (as in torch)
    w = torch.randn(n, generator=gen)
    make = lambda l, h: td.Independent(td.Uniform(l, h, validate_args=False), 1)
    truth = torch_grads(make, (low, high), x, w, torch.float64, 'cpu')
    ref = torch_grads(make, (low, high), x, w, torch.float32, DEV)
    u = st.Uniform(torch.nn.Parameter(low.clone()), torch.nn.Parameter(high.clone())).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    lp = u.log_prob(xd)
    fin = torch.isfinite(lp)
    assert int((~fin).sum()) == 1 and not bool(fin[4])
    (lp[fin] * w.to(DEV)[fin]).sum().backward()
    fin_c = fin.cpu()
    t2 = torch_grads(make, (low, high), x[fin_c], w[fin_c], torch.float64, 'cpu')
    r2 = torch_grads(make, (low, high), x[fin_c], w[fin_c], torch.float32, DEV)
    held('Uniform g_low', u.low.grad, r2[1], t2[1])
    held('Uniform g_high', u.high.grad, r2[2], t2[2])
    assert truth[0] is None and ref[0] is None and torch.equal(xd.grad, torch.zeros_like(xd))      # the indicator has no gradient
    # a one-element parameter broadcast to the row: autograd sums the kernel's column sums back
    s = st.Normal(torch.nn.Parameter(torch.tensor([0.3])), torch.nn.Parameter(torch.tensor([1.7]))).to(DEV)
    xs, ws = torch.randn(33, 5, generator=gen), torch.randn(33, generator=gen)
    (s.log_prob(xs.to(DEV)) * ws.to(DEV)).sum().backward()
    mk = lambda l, sc: td.Independent(td.Normal(l.expand(5), sc.expand(5), validate_args=False), 1)
    t3 = torch_grads(mk, (torch.tensor([0.3]), torch.tensor([1.7])), xs, ws, torch.float64, 'cpu')
    r3 = torch_grads(mk, (torch.tensor([0.3]), torch.tensor([1.7])), xs, ws, torch.float32, DEV)
    held('scalar loc', s.loc.grad, r3[1], t3[1])
    held('scalar scale', s.scale.grad, r3[2], t3[2])


def test_frozen_parameters_and_second_differentiation(monkeypatch):
    """A frozen parameter gets no gradient buffer (its pointer is NULL in the call, no partial buffer when both are frozen); the op is
    differentiable once."""
    gen = ph.generator('bwd/frozen')
    x = torch.randn(33, 5, generator=gen).to(DEV)
    seen = []
    real = _hip.call
    monkeypatch.setattr(_hip, 'call', lambda name, t, *a: (seen.append((name, a)), real(name, t, *a))[1])
    for train_loc, train_scale, train_x in ((True, False, False), (False, True, True), (False, False, True)):
        loc = torch.nn.Parameter(torch.randn(5, generator=gen), requires_grad=train_loc)
        scale = torch.nn.Parameter(0.5 + torch.rand(5, generator=gen), requires_grad=train_scale)
        d = st.Normal(loc, scale).to(DEV)
        xd = x.clone().requires_grad_(train_x)
        seen.clear()
        d.log_prob(xd).sum().backward()
        (name, a), = [s for s in seen if s[0] == 'sx_normal_logprob_bwd']
        gx, g_loc, g_scale, partial = a[4:8]
        assert (gx is not None) == train_x and (g_loc is not None) == train_loc and (g_scale is not None) == train_scale
        assert (partial is not None) == (train_loc or train_scale)
        assert (d.loc.grad is not None) == train_loc and (d.scale.grad is not None) == train_scale and (xd.grad is not None) == train_x
    monkeypatch.undo()
    for d in (st.Normal(torch.zeros(5), torch.ones(5)).to(DEV), st.Uniform(torch.full((5,), -9.0), torch.full((5,), 9.0)).to(DEV)):
        xd = x.clone().requires_grad_(True)
        g, = torch.autograd.grad(d.log_prob(xd).sum(), xd, create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()
    # a multivariate normal with a graph is torch ops end to end: differentiable in x and in its parameters
    tril = torch.nn.Parameter(bh.well_conditioned_tril(5, gen))
    m = st.MultivariateNormal(torch.zeros(5), scale_tril=tril).to(DEV)
    m.log_prob(x).sum().backward()
    assert m.scale_tril.grad is not None and torch.isfinite(m.scale_tril.grad).all()


# ---- flows -------------------------------------------------------------------------------------------------------------------------
def isolated(flow, base_cpu, y):
    """The truth that isolates the base: with (z, log-det) from the product's own inverse pass, truth = ldj + truth_base(z) and the
    reference is the fp32 torch form on the same z.  -> (truth [..., 1], ref [..., 1])"""
    with torch.no_grad():
        z, ldj = flow.inverse_and_log_det_jacobian(y.float())
    t, r = truth_and_ref(base_cpu, z.cpu(), ldj.squeeze(-1))
    return t.unsqueeze(-1), r.unsqueeze(-1)


def big_flow(kind, base_kind, gen, D=64):
    desc = fd.cfg2_desc(2, D, 64) if kind == 'affine' else fd.cfg3_desc(2, D, 64, 8)
    torch.manual_seed(ph.seed_of(f'flow/{kind}'))
    base_cpu = make_dist(base_kind, D, gen)
    if base_kind == 'uniform':
        base_cpu = st.Uniform(torch.full((D,), -40.0), 40.0 + torch.rand(D, generator=gen))
    flow = st.NormalizingFlow(copy.deepcopy(base_cpu), [fd.build_transform(st, d) for d in desc]).to(DEV)
    return flow, base_cpu


@pytest.mark.parametrize('name', bh.FLOW_BASES)
def test_f21_flows(name):
    flow, desc, x, lp32, lp64 = bh.f21_flow(name)
    flow = flow.to(DEV)
    with torch.no_grad():
        got = flow.log_prob(x.to(DEV))
    assert got.shape == (9, 1)
    held(f'F21 flow/{name}', got, lp32, lp64)
    if name != 'uniform':
        assert flow._base_program(6, 0, got.device) is not None                  # one launch


def test_flow_with_a_batch_shaped_base():
    """Parameters outside the kernels' coverage inside a flow: the closed form on the flow's latent, broadcast as in the reference
    (flow.py:129): [3, 1, 6] locs against [9, 6] rows give [3, 9, 1]."""
    flow, desc, x, _, _ = bh.f21_flow('normal')
    gen = ph.generator('flow/batch-shaped')
    base_cpu = st.Normal(torch.randn(3, 1, 6, generator=gen), 0.5 + torch.rand(6, generator=gen))
    flow.base_dist = copy.deepcopy(base_cpu)
    flow = flow.to(DEV)
    with torch.no_grad():
        got = flow.log_prob(x.to(DEV))
        z, ldj = flow.inverse_and_log_det_jacobian(x.to(DEV))
        t = bh.torch_dist(base_cpu).log_prob(z.cpu().double()).unsqueeze(-1) + ldj.cpu().double()
        r = bh.torch_dist(base_cpu, torch.float32, DEV).log_prob(z).unsqueeze(-1) + ldj
        assert got.shape == (3, 9, 1)
        held('batch-shaped Normal base in a flow', got, r, t)
        total = flow.log_prob_sum(x.to(DEV))
        assert abs(total.item() - got.double().sum().item()) <= 1e-9 * abs(got.double().sum().item())


@pytest.mark.parametrize('kind,base_kind', [('affine', 'normal'), ('affine', 'mvn'), ('rqs', 'normal'), ('rqs', 'uniform'), ('rqs', 'mvn')])
def test_flow_log_prob_and_sum(kind, base_kind):
    """D = 64, two couplings.  Affine flows with a Normal / MultivariateNormal base run as ONE program; Uniform, and the multivariate
    normal behind splines (a dense step beside spline steps does not plan), take the two-launch form.  Same values within the bound,
    fp32 and bf16 storage; log_prob_sum = the fp64 sum of log_prob within 1e-9 relative."""
    gen = ph.generator(f'flow/{kind}/{base_kind}')
    flow, base_cpu = big_flow(kind, base_kind, gen)
    y = torch.randn(130, 64, generator=gen).to(DEV)
    with torch.no_grad():
        prog = flow._base_program(64, 0, y.device) if hasattr(flow.base_dist, '_plan') else None
        if kind == 'affine':
            assert prog is not None                  # ONE program: the transforms' steps and the base as a trailing step
            assert prog.prog.n_steps == flow._fused_program(True, 64, 0, y.device).prog.n_steps + 1
        if base_kind == 'uniform' or (kind, base_kind) == ('rqs', 'mvn'):
            assert prog is None                      # two launches
        got = flow.log_prob(y)
        t, r = isolated(flow, base_cpu, y)
        assert got.shape == (130, 1) and got.dtype == torch.float32
        held(f'{kind}/{base_kind} log_prob', got, r, t)
        got3 = flow.log_prob(y.reshape(2, 65, 64))
        assert got3.shape == (2, 65, 1) and torch.equal(got3.reshape(130, 1), got)
        total = flow.log_prob_sum(y)
        want = got.double().sum().item()
        assert total.dtype == torch.float64 and abs(total.item() - want) <= 1e-9 * abs(want), (total.item(), want)
        out = torch.full((1,), 2.5, dtype=torch.float64, device=DEV)
        assert flow.log_prob_sum(y, out=out) is out and abs(out.item() - 2.5 - want) <= 1e-9 * abs(want)
        yb = y.bfloat16()
        tb, rb = isolated(flow, base_cpu, yb)
        held(f'{kind}/{base_kind} log_prob bf16', flow.log_prob(yb), rb, tb)
        for s in (flow.sample(5), flow.sample((2, 3)), flow.rsample(5), flow.sample(5, rsample=True)):
            assert s.device.type == 'cuda' and s.shape[-1] == 64 and s.shape[0] in (5, 2) and torch.isfinite(s).all()


@pytest.mark.parametrize('base_kind', ['normal', 'mvn', 'uniform'])
def test_parameter_updates_reach_the_next_call(base_kind):
    """A changed parameter reaches the next log_prob: an in-place update under no_grad, and `loc.data.add_(1)` followed by an
    optimizer step.  (Programs and operands are guarded on the parameters' (data_ptr, _version), like every parameter in this
    library; an edit through `.data` alone does not bump `_version` -- it is seen with the next update that does, here the step.)"""
    gen = ph.generator(f'update/{base_kind}')
    flow, base_cpu = big_flow('affine', base_kind, gen)
    base = flow.base_dist
    first = 'low' if base_kind == 'uniform' else 'loc'
    for name, buf in list(base.named_buffers()):
        delattr(base, name)
        base.register_parameter(name, torch.nn.Parameter(buf.clone()))
    y = torch.randn(33, 64, generator=gen).to(DEV)

    def check(tag):
        with torch.no_grad():
            got = flow.log_prob(y)
            now = copy.deepcopy(base).cpu()
            t, r = isolated(flow, now, y)
        held(f'{base_kind} {tag}', got, r, t)
        return got
    lp0 = check('before')
    with torch.no_grad():
        getattr(base, first).add_(0.25)
    lp1 = check('after an in-place update')
    assert not torch.equal(lp0, lp1)
    getattr(base, first).data.add_(1)
    opt = torch.optim.SGD(flow.parameters(), lr=1e-3)
    (-flow.log_prob(y).mean()).backward()
    assert all(p.grad is not None for p in base.parameters())
    opt.step()
    lp2 = check('after .data.add_(1) and an optimizer step')
    assert not torch.equal(lp1, lp2)
    if base_kind != 'uniform':                       # the shift by 1 is in what the next call used
        assert (lp2 - lp1).abs().max().item() > 1e-2


def test_one_training_step_with_a_learnable_normal_base():
    """-log_prob.mean() of the D = 64 affine flow with a learnable Normal base: every gradient against the fp64 oracle (the base's
    closed form on the oracle's latent; e_ref: the same in fp32 on the CPU), and the couplings' gradients unchanged against the same
    flow written with a leading Affine(scale, shift=loc) layer and a UnitNormal base, within the same bound."""
    import torch.distributions as td
    gen = ph.generator('train')
    flow, base_cpu = big_flow('affine', 'normal', gen)
    desc = fd.cfg2_desc(2, 64, 64)
    base = flow.base_dist
    loc0, scale0 = base.loc.detach().clone(), base.scale.detach().clone()
    del base.loc, base.scale
    base.loc, base.scale = torch.nn.Parameter(loc0.clone()), torch.nn.Parameter(scale0.clone())
    y = torch.randn(130, 64, generator=gen).to(DEV)
    lp = flow.log_prob(y)
    assert lp.requires_grad and lp.shape == (130, 1)
    (-lp.mean()).backward()
    got = {k: p.grad for k, p in flow.named_parameters()}
    assert set(got) >= {'base_dist.loc', 'base_dist.scale'} and all(g is not None for g in got.values())

    def oracle_grads(dtype):
        state = {k: p.detach().cpu().to(dtype).requires_grad_(True) for k, p in flow.named_parameters()}
        spec = fd.flow_spec(desc, state)
        z, ldj = orc.flow_inverse_and_ldj(spec, y.cpu().to(dtype))
        b = td.Independent(td.Normal(state['base_dist.loc'], state['base_dist.scale'], validate_args=False), 1)
        (-(b.log_prob(z).unsqueeze(-1) + ldj).mean()).backward()
        return {k: v.grad for k, v in state.items()}
    truth, ref = oracle_grads(torch.float64), oracle_grads(torch.float32)
    # the same flow with the base written as a layer
    twin = st.NormalizingFlow(st.UnitNormal(64), [st.Affine(64, scale=scale0.cpu(), shift=loc0.cpu())]
                              + [copy.deepcopy(f) for f in flow.transforms]).to(DEV)
    for p in twin.parameters():
        p.grad = None
    (-twin.log_prob(y).mean()).backward()
    twin_grads = {k: p.grad for k, p in twin.named_parameters()}
    for k in sorted(got):
        held(f'train {k}', got[k], ref[k], truth[k])
        if k.startswith('transforms.'):
            i, rest = k[len('transforms.'):].split('.', 1)
            other = twin_grads[f'transforms.{int(i) + 1}.{rest}']
            tol, _ = ch.bound(ref[k], truth[k])
            diff = (got[k] - other).abs().max().item()
            print(f'train {k}: |with base - with Affine layer| {diff:.3e} bound {tol:.3e}')
            assert diff <= tol, (k, diff, tol)
    with torch.no_grad():
        assert torch.isfinite(flow.log_prob(y)).all()
    st.check_errors()
