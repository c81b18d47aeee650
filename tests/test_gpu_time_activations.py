"""GPU: ContinuousTanh / ContinuousActivation (sx_pointwise_time and its backward), the same two as steps of the one-launch NeuralFlow
program, CumsumColumn / DiffColumn and net.ResNet.

Against fixture F24 (the reference's recorded fp32 results) and against the fp64 truth -- the reference's literal sequences evaluated in
fp64 on the CPU (timeacthelp).  The tolerance is the project's measured one, cnfhelp.bound: 8 x the reference's own fp32 error (over the
entries where its fp32 result is finite), floored at 1e-6 * max(1, max |truth|); a bf16 output additionally gets half a bf16 ulp
(storagehelp).  The kernel states the tanh-flow in the log domain, so it must be finite -- and within that bound -- where the reference's
fp32 sequence overflows."""
import warnings

import pytest
import torch

import timeacthelp as th
from storagehelp import assert_store, offset_view

import stribor_amd as st

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROWS = (1, 63, 65, 1000)            # one row, a partial wave, one past a wave, several workgroups
DIMS = (1, 5, 32, 33, 130)          # scalar lanes, ragged rows, 16-byte lanes, one past them, rows wider than two waves (8-wide bf16 lanes)
SETS = {1: (1, 1), 63: (7, 9), 65: (5, 13), 1000: (8, 125)}


def close(got, want, rtol=1e-5, atol=1e-5):
    torch.testing.assert_close(got.detach().cpu().float(), want, rtol=rtol, atol=atol)


def held(got, ref32, truth64, what):
    """assert_store under timeacthelp.bound (reference error over its finite entries); the result itself must be finite."""
    assert torch.isfinite(got.float()).all(), f'{what}: non-finite result'
    fin = torch.isfinite(ref32)
    assert_store(got, torch.where(fin, ref32, truth64.float()), truth64, what, tol=th.bound(ref32, truth64))


# ---- fixture parity ------------------------------------------------------------------------------------------------------------------
def test_fixture_parity_tanh_and_activation():
    g = th.golden()
    with torch.no_grad():
        x, t = g.t('tanh/x').to(DEV), g.t('tanh/t').to(DEV)
        for lt in (0, 1):
            f = st.ContinuousTanh(log_time=bool(lt))
            y = f(x, t)
            close(y, g.t(f'tanh/log{lt}/y'))
            close(f.inverse(g.t(f'tanh/log{lt}/y').to(DEV), t), g.t(f'tanh/log{lt}/x_back'))
            close(f.forward(y, t, reverse=True), g.t(f'tanh/log{lt}/x_back'))
            ld = f.log_diag_jacobian(x, y, t)
            close(ld, g.t(f'tanh/log{lt}/ldiag'))
            close(f.log_det_jacobian(x, y, t), g.t(f'tanh/log{lt}/ldiag').sum(-1, keepdim=True), atol=3e-5)
            y2, ldj = f.forward_and_log_det_jacobian(x, t=t)
            assert torch.equal(y2, y) and ldj.shape == (13, 3, 1)
            xb, ldj_inv = f.inverse_and_log_det_jacobian(y, t=t)
            close(xb, x.cpu(), atol=2e-5)
            close(ldj_inv, -ldj.cpu(), atol=3e-5)                      # flow.py:42-47: minus the forward log-det at the value produced
            y3, ld3 = f.forward_and_log_diag_jacobian(x, t=t)
            assert torch.equal(y3, y) and torch.equal(ld3, ld)
            xb2, ld_inv = f.inverse_and_log_diag_jacobian(y, t=t)
            assert torch.equal(xb2, xb)
            close(ld_inv, -ld.cpu(), atol=2e-5)
        x, tr = g.t('act/x').to(DEV), g.t('act/t_rand').to(DEV)
        for name, fn in th.ACTS.items():
            for temp in (1.0, 2.5):
                f = st.ContinuousActivation(fn, temperature=temp).to(DEV)
                assert torch.equal(f(x, torch.zeros_like(tr)), x)      # identity at t = 0, bit for bit
                close(f(x, tr), g.t(f'act/{name}/T{temp:g}/y_rand'))
                close(f(x, torch.full_like(tr, 100.0)), g.t(f'act/{name}/T{temp:g}/y_100'))
                twin = {'tanh': torch.nn.Tanh(), 'sigmoid': torch.nn.functional.sigmoid, 'relu': torch.nn.ReLU()}[name]
                assert torch.equal(st.ContinuousActivation(twin, temperature=temp).to(DEV)(x, tr), f(x, tr))


def test_time_shapes_and_torch_op_routes():
    """One time per row in every broadcastable form takes the kernel; a feature axis of width dim and an uncovered callable run the
    reference's lines as torch ops on the device."""
    torch.manual_seed(1)
    with torch.no_grad():
        x = torch.randn(4, 3, 5) * 2
        f, a = st.ContinuousTanh(), st.ContinuousActivation(torch.tanh, 2.0).to(DEV)
        per_row = torch.rand(4, 3, 1) * 3
        want = f(x.to(DEV), per_row.to(DEV))
        for t in (torch.tensor(1.5), torch.tensor([1.5]), torch.full((3, 1), 1.5), torch.full((4, 1, 1), 1.5)):
            tt = t.expand(4, 3, 1) if t.dim() else t.reshape(1, 1, 1).expand(4, 3, 1)
            held(f(x.to(DEV), t.to(DEV)), th.tanh_flow(x, tt), th.tanh_flow(x.double(), tt.double()), f'tanh t{tuple(t.shape)}')
            held(a(x.to(DEV), t.to(DEV)), th.mix('tanh', x, tt, torch.tensor(2.0)), th.mix('tanh', x.double(), tt.double(), 2.0), f'act t{tuple(t.shape)}')
        per_set = torch.rand(4, 1, 1) * 3
        assert torch.equal(f(x.to(DEV), per_set.to(DEV)), f(x.to(DEV), per_set.expand(4, 3, 1).contiguous().to(DEV)))
        assert torch.equal(f(x.to(DEV), 1.5), f(x.to(DEV), torch.tensor(1.5, device=DEV)))
        # per-feature times: torch ops
        tf = torch.rand(4, 3, 5) * 3
        close(f(x.to(DEV), tf.to(DEV)), th.tanh_flow(x, tf))
        close(f.log_diag_jacobian(x.to(DEV), None, tf.to(DEV)), th.tanh_flow_ldiag(x, tf))
        close(a(x.to(DEV), tf.to(DEV)), th.mix('tanh', x, tf, torch.tensor(2.0)))
        # an uncovered callable
        s = st.ContinuousActivation(torch.sin, 2.0).to(DEV)
        w = torch.tanh(2.0 * per_row)
        close(s(x.to(DEV), per_row.to(DEV)), x * (1 - w) + torch.sin(x) * w)
        assert want.shape == x.shape


# ---- the sweep against the fp64 truth ----------------------------------------------------------------------------------------------
def put(v, bf, k):
    v = (v.bfloat16() if bf else v).to(DEV)
    return offset_view(v, k) if k else v


@pytest.mark.parametrize('dim', DIMS)
@pytest.mark.parametrize('rows', ROWS)
def test_sweep_against_fp64(rows, dim):
    g = torch.Generator().manual_seed(100 * rows + dim)
    B, S = SETS[rows]
    with torch.no_grad():
        x32 = torch.randn(B, S, dim, generator=g) * 3
        t_row = torch.rand(B, S, 1, generator=g) * 5
        t_set = torch.rand(B, 1, 1, generator=g) * 5
        times = {'row': t_row, 'set': t_set, 'scalar': torch.tensor(1.25), 'zero': torch.zeros(B, S, 1)}
        for bf in (False, True):
            xs = x32.bfloat16().float() if bf else x32              # the values the kernel sees
            for k in (0, 1):
                xd = put(x32, bf, k)
                for tname, t in times.items():
                    if k and tname not in ('row',):
                        continue
                    te = t.expand(B, S, 1) if t.dim() else t.reshape(1, 1, 1).expand(B, S, 1)
                    td = t.to(DEV)
                    tag = f'[{rows}x{dim} {"bf16" if bf else "f32"} +{k} t={tname}]'
                    for lt in (False, True):
                        f = st.ContinuousTanh(lt)
                        y, ld = f.forward_and_log_diag_jacobian(xd, t=td)
                        assert y.dtype == xd.dtype and ld.dtype == torch.float32
                        y64, ld64 = th.tanh_flow(xs.double(), te.double(), lt), th.tanh_flow_ldiag(xs.double(), te.double(), lt)
                        held(y, th.tanh_flow(xs, te, lt), y64, f'tanh{int(lt)} y {tag}')
                        held(ld, th.tanh_flow_ldiag(xs, te, lt), ld64, f'tanh{int(lt)} ldiag {tag}')
                        _, ldj = f.forward_and_log_det_jacobian(xd, t=td)
                        held(ldj, th.tanh_flow_ldiag(xs, te, lt).sum(-1, keepdim=True), ld64.sum(-1, keepdim=True), f'tanh{int(lt)} ldj {tag}')
                        xb, ldi = f.inverse_and_log_diag_jacobian(xd, t=td)
                        held(xb, th.tanh_flow(xs, te, lt, True), th.tanh_flow(xs.double(), te.double(), lt, True), f'tanh{int(lt)} inverse {tag}')
                        held(ldi, th.tanh_flow_ldiag(xs, te, lt, True), th.tanh_flow_ldiag(xs.double(), te.double(), lt, True), f'tanh{int(lt)} inverse ldiag {tag}')
                        if tname == 'zero':
                            held(y, xs, xs.double(), f'tanh{int(lt)} identity at t = 0 {tag}')
                    for name, fn in th.ACTS.items():
                        f = st.ContinuousActivation(fn, 2.5).to(DEV)
                        y = f(xd, td)
                        held(y, th.mix(name, xs, te, torch.tensor(2.5)), th.mix(name, xs.double(), te.double(), 2.5), f'{name} {tag}')
                        if tname == 'zero':
                            assert torch.equal(y, xd), f'{name} identity at t = 0 {tag}'


# ---- the two domains -----------------------------------------------------------------------------------------------------------------
def test_domain_one_reference_finite():
    torch.manual_seed(7)
    with torch.no_grad():
        x = torch.randn(257, 33) * 8
        t = torch.rand(257, 1) * 5
        f = st.ContinuousTanh()
        ref_y, ref_ld = th.tanh_flow(x, t), th.tanh_flow_ldiag(x, t)
        assert torch.isfinite(ref_y).all() and torch.isfinite(ref_ld).all()
        y, ld = f.forward_and_log_diag_jacobian(x.to(DEV), t=t.to(DEV))
        held(y, ref_y, th.tanh_flow(x.double(), t.double()), 'domain 1 y')
        held(ld, ref_ld, th.tanh_flow_ldiag(x.double(), t.double()), 'domain 1 ldiag')
        held(f.inverse(y, t.to(DEV)), th.tanh_flow(ref_y, t, reverse=True), x.double(), 'domain 1 round trip')


def test_domain_two_overflow_band():
    torch.manual_seed(8)
    with torch.no_grad():
        x = torch.randn(257, 33) * 30
        x[0, :7] = torch.tensor([95.0, -95.0, 88.0, -60.0, 44.0, 1e-3, 0.0])
        t = torch.full((257, 1), 5.0)
        ref_y, ref_ld = th.tanh_flow(x, t), th.tanh_flow_ldiag(x, t)
        bad = (~torch.isfinite(ref_y)) | (~torch.isfinite(ref_ld))
        print(f'reference non-finite on {bad.float().mean().item():.3f} of the band')
        assert 0.1 < bad.float().mean().item() < 0.4
        for lt in (False, True):
            f = st.ContinuousTanh(lt)
            y, ld = f.forward_and_log_diag_jacobian(x.to(DEV), t=t.to(DEV))
            assert torch.isfinite(y).all() and torch.isfinite(ld).all()
            held(y, th.tanh_flow(x, t, lt), th.tanh_flow(x.double(), t.double(), lt), f'band y log_time={lt}')
            held(ld, th.tanh_flow_ldiag(x, t, lt), th.tanh_flow_ldiag(x.double(), t.double(), lt), f'band ldiag log_time={lt}')
            back = f.inverse(y, t.to(DEV))
            held(back, th.tanh_flow(th.tanh_flow(x, t, lt), t, lt, True), x.double(), f'band round trip log_time={lt}')
            _, ldj = f.forward_and_log_det_jacobian(x.to(DEV), t=t.to(DEV))
            held(ldj, th.tanh_flow_ldiag(x, t, lt).sum(-1, keepdim=True), th.tanh_flow_ldiag(x.double(), t.double(), lt).sum(-1, keepdim=True),
                 f'band ldj log_time={lt}')
        xb = x.bfloat16()
        y = st.ContinuousTanh()(xb.to(DEV), t.to(DEV))
        held(y, th.tanh_flow(xb.float(), t), th.tanh_flow(xb.double(), t.double()), 'band y bf16')


# ---- gradients -----------------------------------------------------------------------------------------------------------------------
def grad_held(got, ref32, truth64, what):
    assert got.dtype == torch.float32
    held(got, ref32.float(), truth64, what)


@pytest.mark.parametrize('rows,dim', [(1, 1), (63, 5), (65, 33), (257, 32), (100, 130)])
def test_tanh_flow_gradients(rows, dim):
    g = torch.Generator().manual_seed(rows + dim)
    x = torch.randn(rows, dim, generator=g) * 3
    t = torch.rand(rows, 1, generator=g) * 5
    gy, gld = torch.randn(rows, dim, generator=g), torch.randn(rows, dim, generator=g)
    for lt in (False, True):
        for reverse in (False, True):
            f = st.ContinuousTanh(lt)
            xd, td = x.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
            y, ld = (f.inverse_and_log_diag_jacobian if reverse else f.forward_and_log_diag_jacobian)(xd, t=td)
            loss = (y * gy.to(DEV)).sum() + (ld * gld.to(DEV)).sum()
            gx, gt = torch.autograd.grad(loss, (xd, td), retain_graph=True)
            gx2, gt2 = torch.autograd.grad(loss, (xd, td))
            assert torch.equal(gx, gx2) and torch.equal(gt, gt2)          # no atomics: the same bits
            r32, r64 = th.flow_grads(x, t, gy, gld, lt, reverse, torch.float32), th.flow_grads(x, t, gy, gld, lt, reverse, torch.float64)
            tag = f'[{rows}x{dim} log_time={lt} reverse={reverse}]'
            grad_held(gx, r32[0], r64[0], f'gx {tag}')
            grad_held(gt, r32[1], r64[1], f'gt {tag}')
    # the row log-det alone (gldj), and x alone (no time gradient asked for)
    f = st.ContinuousTanh()
    xd = x.to(DEV).requires_grad_(True)
    gl = torch.randn(rows, 1, generator=g)
    (gx,) = torch.autograd.grad((f.log_det_jacobian(xd, None, t.to(DEV)) * gl.to(DEV)).sum(), xd)
    z = torch.zeros_like(gy)
    r32, r64 = th.flow_grads(x, t, z, gl.expand(rows, dim), False, False, torch.float32), th.flow_grads(x, t, z, gl.expand(rows, dim), False, False, torch.float64)
    grad_held(gx, r32[0], r64[0], f'gx of the row log-det [{rows}x{dim}]')


@pytest.mark.parametrize('name', sorted(th.ACTS))
@pytest.mark.parametrize('rows,dim', [(1, 1), (65, 33), (1000, 130)])
def test_mix_gradients(rows, dim, name):
    g = torch.Generator().manual_seed(rows + dim)
    x = torch.randn(rows, dim, generator=g) * 2
    t = torch.rand(rows, 1, generator=g) * 2
    gy = torch.randn(rows, dim, generator=g)
    f = st.ContinuousActivation(th.ACTS[name], temperature=0.75, learnable=True).to(DEV)
    xd, td = x.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    loss = (f(xd, td) * gy.to(DEV)).sum()
    got = torch.autograd.grad(loss, (xd, td, f.temperature), retain_graph=True)
    again = torch.autograd.grad(loss, (xd, td, f.temperature))
    assert all(torch.equal(a, b) for a, b in zip(got, again))             # fixed-order partials + one ordered reduce
    r32, r64 = th.mix_grads(name, x, t, 0.75, gy, torch.float32), th.mix_grads(name, x, t, 0.75, gy, torch.float64)
    for a, b, c, what in zip(got, r32, r64, ('gx', 'gt', 'gtemperature')):
        assert a.shape == c.shape
        grad_held(a, b, c, f'{what} {name} [{rows}x{dim}]')
    # learnable=False: x and t still carry gradients, the temperature none
    f2 = st.ContinuousActivation(th.ACTS[name], temperature=0.75).to(DEV)
    gx, gt = torch.autograd.grad((f2(xd, td) * gy.to(DEV)).sum(), (xd, td))
    assert torch.equal(gx, got[0]) and torch.equal(gt, got[1])


def test_gradients_finite_at_t_100():
    """The reference's check_gradients_not_nan case: t = 100."""
    torch.manual_seed(3)
    x = (torch.randn(10, 4, 5) * 2).to(DEV).requires_grad_(True)
    t = torch.full((10, 4, 1), 100.0, device=DEV, requires_grad=True)
    for f in (st.ContinuousTanh(), st.ContinuousTanh(True), st.ContinuousActivation(torch.tanh, learnable=True).to(DEV),
              st.ContinuousActivation(torch.relu, 2.5, learnable=True).to(DEV)):
        y = f(x, t=t)
        ps = [p for p in f.parameters() if p.requires_grad]
        gs = torch.autograd.grad(y.sum(), [x, t] + ps)
        assert torch.isfinite(y).all() and all(torch.isfinite(g_).all() for g_ in gs), type(f).__name__
    f = st.ContinuousTanh()
    y, ldj = f.forward_and_log_det_jacobian(x, t=t)
    gs = torch.autograd.grad(y.sum() + ldj.sum(), (x, t))
    assert torch.isfinite(ldj).all() and all(torch.isfinite(g_).all() for g_ in gs)


# ---- the fused flow ------------------------------------------------------------------------------------------------------------------
def layer_by_layer(nf, x, t, t0=None, **kw):
    if t0 is not None:
        for f in reversed(nf.transforms):
            x = f.inverse(x, t=t0, **kw)
    for f in nf.transforms:
        x = f(x, t=t, **kw)
    return x


@pytest.mark.parametrize('dim,rows,latent', [(1, 64, 0), (6, 257, 0), (6, 64, 3), (33, 257, 0), (96, 64, 0), (96, 257, 0)])
def test_fused_mixed_flow(dim, rows, latent):
    with torch.no_grad():
        g = torch.Generator().manual_seed(dim + rows)
        x = torch.randn(rows, dim, generator=g)
        t, t0 = torch.rand(rows, 1, generator=g) * 2, torch.rand(rows, 1, generator=g) * 2
        lat = torch.randn(rows, latent, generator=g) if latent else None
        kw = {} if lat is None else {'latent': lat.to(DEV)}
        for last in (True, False):
            nf, descs = th.mixed_flow(dim, latent, last=last, seed=dim)
            state = {k: v.clone() for k, v in nf.state_dict().items()}
            nf = nf.to(DEV)
            t0_ = None if last else t0
            assert nf._fused(dim, latent, t0_ is not None, torch.device(DEV, 0)) is not None, (dim, last)
            got = nf(x.to(DEV), t.to(DEV), None if t0_ is None else t0_.to(DEV), **kw)
            ref = layer_by_layer(nf, x.to(DEV), t.to(DEV), None if t0_ is None else t0_.to(DEV), **kw)
            truth = th.mixed_flow_eval(descs, state, x, t, t0_, lat)
            held(got, ref.cpu().float(), truth, f'fused mixed flow dim {dim} rows {rows} latent {latent} {"t" if last else "t, t0"}')
            zero = nf(x.to(DEV), torch.zeros_like(t).to(DEV), **kw)
            assert (zero.cpu() - x).abs().max().item() <= 1e-6, 'identity at t = 0'
            if not last:
                back = nf(x.to(DEV), t0.to(DEV), t0.to(DEV), **kw)              # test_neural_flow.py:29-32
                assert (back.cpu() - x).abs().max().item() <= 1e-4
        # bf16 storage rides through the same program
        nf, descs = th.mixed_flow(dim, latent, seed=dim)
        state = {k: v.clone() for k, v in nf.state_dict().items()}
        nf = nf.to(DEV)
        xb = x.bfloat16()
        got = nf(xb.to(DEV), t.to(DEV), **kw)
        ref = layer_by_layer(nf, xb.float().to(DEV), t.to(DEV), **kw)
        held(got, ref.cpu().float(), th.mixed_flow_eval(descs, state, xb.float(), t, None, lat), f'fused mixed flow dim {dim} bf16')


def test_fused_flow_fixture_and_temperature_guard():
    g = th.golden()
    with torch.no_grad():
        x, t, t0 = (g.t('flow/' + k).to(DEV) for k in ('x', 't', 't0'))
        nf, _ = th.mixed_flow(6)
        nf.load_state_dict(g.state('flow'))
        nf = nf.to(DEV)
        assert nf._fused(6, 0, False, x.device) is not None
        close(nf(x, t=t), g.t('flow/y_t'), atol=2e-5)
        with pytest.raises(NotImplementedError):
            nf(x, t=t, t0=t0)
        nf3, _ = th.mixed_flow(6, last=False)
        nf3.load_state_dict({k: v for k, v in g.state('flow').items() if not k.startswith('transforms.3.')})
        nf3 = nf3.to(DEV)
        assert nf3._fused(6, 0, True, x.device) is not None
        close(nf3(x, t=t, t0=t0), g.t('flow/y_t_t0'), atol=2e-5)
        # the temperature is baked into the step: an in-place change re-plans
        before = nf(x, t=t)
        nf.transforms[3].temperature.fill_(2.5)
        after = nf(x, t=t)
        assert not torch.equal(before, after)
        close(after, layer_by_layer(nf, x, t).cpu(), atol=2e-5)
        # a learnable temperature wants a graph: layer by layer, differentiable
    nf.transforms[3].temperature.requires_grad_(True)
    y = nf(x, t=t)
    (gtemp,) = torch.autograd.grad(y.sum(), nf.transforms[3].temperature)
    assert torch.isfinite(gtemp) and gtemp.shape == ()


def test_pointwise_only_neural_flow_and_per_feature_times():
    """A NeuralFlow without a coupling is a program of SX_STEP_POINTWISE_TIME steps alone (its first step is a point-wise one); a t with a
    feature axis leaves the one-launch path for the layers' torch ops."""
    with torch.no_grad():
        for dim, rows in ((5, 65), (33, 257), (96, 64)):
            g = torch.Generator().manual_seed(dim)
            x = torch.randn(rows, dim, generator=g) * 2
            t, t0 = torch.rand(rows, 1, generator=g) * 3, torch.rand(rows, 1, generator=g) * 3
            nf = st.NeuralFlow([st.ContinuousTanh(True), st.ContinuousActivation(torch.nn.functional.relu, 2.5)]).to(DEV)
            prog = nf._fused(dim, 0, False, torch.device(DEV, 0))
            assert prog is not None and [prog.prog.steps[i].kind for i in range(prog.prog.n_steps)] == [25, 25]
            got = nf(x.to(DEV), t.to(DEV))

            def both(v, tt, dt):
                return th.mix('relu', th.tanh_flow(v.to(dt), tt.to(dt), True), tt.to(dt), torch.tensor(2.5, dtype=dt))
            held(got, both(x, t, torch.float32), both(x, t, torch.float64), f'point-wise only flow dim {dim}')
            assert torch.equal(nf(x.to(DEV), torch.zeros_like(t).to(DEV)).cpu(), x)
            solo = st.NeuralFlow([st.ContinuousTanh()])
            assert solo._fused(dim, 0, True, torch.device(DEV, 0)) is not None
            got = solo(x.to(DEV), t.to(DEV), t0.to(DEV))

            def there(v, dt):
                return th.tanh_flow(th.tanh_flow(v.to(dt), t0.to(dt), False, True), t.to(dt))
            held(got, there(x, torch.float32), there(x, torch.float64), f'tanh-flow t0 -> t dim {dim}')
            # per-feature times: no fused program is taken, the layers run the reference's lines
            tf = torch.rand(rows, dim, generator=g) * 3
            close(nf(x.to(DEV), tf.to(DEV)), th.mix('relu', th.tanh_flow(x, tf, True), tf, torch.tensor(2.5)))
            close(solo(x.to(DEV), tf.to(DEV), tf.to(DEV)), x, atol=2e-5)


def test_normalizing_flow_trains_through_continuous_tanh():
    """NormalizingFlow hands `t` to ContinuousTanh on its layer-wise autograd path: forward / inverse with their log-dets and log_prob
    are differentiable in x and t; against fp64 autograd of the restatement under the measured bound."""
    g = torch.Generator().manual_seed(11)
    B, S, D = 5, 13, 6
    x = torch.randn(B, S, D, generator=g) * 2
    gy, gl = torch.randn(B, S, D, generator=g), torch.randn(B, S, 1, generator=g)
    flow = st.NormalizingFlow(st.UnitNormal(D), [st.ContinuousTanh(), st.Flip(), st.ContinuousTanh(True)])

    def restated(xv, tv, what, dt):
        xv, tv = xv.detach().to(dt).requires_grad_(True), tv.detach().to(dt).requires_grad_(True)
        te = tv.expand(B, S, tv.shape[-1])
        if what == 'forward':
            y1 = th.tanh_flow(xv, te)
            y2 = th.tanh_flow(y1.flip(-1), te, True)
            ldj = th.tanh_flow_ldiag(xv, te).sum(-1, keepdim=True) + th.tanh_flow_ldiag(y1.flip(-1), te, True).sum(-1, keepdim=True)
            loss = (y2 * gy.to(dt)).sum() + (ldj * gl.to(dt)).sum()
        else:
            x1 = th.tanh_flow(xv, te, True, True)
            x0 = th.tanh_flow(x1.flip(-1), te, False, True)
            ldj = th.tanh_flow_ldiag(xv, te, True, True).sum(-1, keepdim=True) + th.tanh_flow_ldiag(x1.flip(-1), te, False, True).sum(-1, keepdim=True)
            if what == 'inverse':
                loss = (x0 * gy.to(dt)).sum() + (ldj * gl.to(dt)).sum()
            else:
                logp = -0.5 * (x0 * x0).sum(-1, keepdim=True) - 0.5 * D * torch.log(torch.tensor(2 * torch.pi, dtype=dt)) + ldj
                loss = (logp * gl.to(dt)).sum()
        return torch.autograd.grad(loss, (xv, tv))

    for tname, t in (('row', torch.rand(B, S, 1, generator=g) * 3), ('set', torch.rand(B, 1, 1, generator=g) * 3),
                     ('feature', torch.rand(B, S, D, generator=g) * 2)):
        for what in ('forward', 'inverse', 'log_prob'):
            xd, td = x.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
            with warnings.catch_warnings():
                warnings.filterwarnings('error', message='.*WITHOUT an autograd graph.*')      # the graph is really built
                if what == 'forward':
                    y, ldj = flow.forward_and_log_det_jacobian(xd, t=td)
                    loss = (y * gy.to(DEV)).sum() + (ldj * gl.to(DEV)).sum()
                elif what == 'inverse':
                    y, ldj = flow.inverse_and_log_det_jacobian(xd, t=td)
                    loss = (y * gy.to(DEV)).sum() + (ldj * gl.to(DEV)).sum()
                else:
                    loss = (flow.log_prob(xd, t=td) * gl.to(DEV)).sum()
            gx, gt = torch.autograd.grad(loss, (xd, td))
            r32, r64 = restated(x, t, what, torch.float32), restated(x, t, what, torch.float64)
            assert gt.shape == t.shape
            held(gx, r32[0].float(), r64[0], f'NormalizingFlow {what} gx t={tname}')
            held(gt, r32[1].float(), r64[1], f'NormalizingFlow {what} gt t={tname}')
    # ContinuousActivation has no log-det: a NormalizingFlow that holds it leaves as in the reference
    bad = st.NormalizingFlow(st.UnitNormal(D), [st.ContinuousActivation(torch.tanh).to(DEV)])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(NotImplementedError):
            bad.log_prob(x.to(DEV).requires_grad_(True), t=torch.rand(B, S, 1, device=DEV))


# ---- CumsumColumn / DiffColumn, net.ResNet -----------------------------------------------------------------------------------------------
def test_cumsum_column_and_resnet():
    g = th.golden()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        cols = {c: (st.CumsumColumn(c), st.DiffColumn(c)) for c in (0, 2)}
    with torch.no_grad():
        x = g.t('column/x').to(DEV)
        for c, (cs, df) in cols.items():
            y = cs(x)
            close(y, g.t(f'column/c{c}/cumsum'), atol=1e-6)
            close(df(x), g.t(f'column/c{c}/diff'), atol=1e-6)
            close(cs.inverse(y), x.cpu(), atol=1e-6)
            close(df.inverse(df(x)), x.cpu(), atol=1e-6)
            keep = [k for k in range(3) if k != c]
            assert torch.equal(y[..., keep], x[..., keep])
            assert torch.equal(cs.log_det_jacobian(x, y), torch.zeros(2, 6, 1, device=DEV))
            assert torch.equal(cs.log_diag_jacobian(x, y), torch.zeros_like(x))
            yi, ldj = cs.forward_and_log_det_jacobian(x)
            assert torch.equal(yi, y) and not ldj.any()
        big = torch.randn(3, 70, 5, device=DEV)
        close(cols[2][0](big), torch.cat([big[..., :2], big[..., 2].cumsum(-1).unsqueeze(-1), big[..., 3:]], -1).cpu(), atol=1e-5)
    xg = g.t('column/x').to(DEV).requires_grad_(True)
    (gx,) = torch.autograd.grad((cols[0][0](xg) * torch.arange(3.0, device=DEV)).sum(), xg)
    xc = g.t('column/x').requires_grad_(True)
    yc = xc.clone()
    yc[..., 0] = yc[..., 0].cumsum(-1)
    (gc,) = torch.autograd.grad((yc * torch.arange(3.0)).sum(), xc)
    close(gx, gc, atol=1e-6)

    with torch.no_grad():
        net = st.net.ResNet(4, [7, 5], 3)
        net.load_state_dict(g.state('resnet'))
        close(net.to(DEV)(g.t('resnet/x').to(DEV)), g.t('resnet/y'), atol=2e-5)
        # as the conditioner of a Coupling (the any-nn.Module tier), against its torch evaluation in fp64
        torch.manual_seed(5)
        D = 6
        cond = torch.nn.Sequential(st.net.ResNet(D, [9], 2, activation='Tanh'), torch.nn.Linear(D, 2 * D))
        layer = st.Coupling(st.Affine(D, latent_net=cond), mask='ordered_left_half')
        x = torch.randn(65, D)
        from oracle import stribor_oracle as orc
        m = orc.mask_vector('ordered_left_half', D).double()
        r = x.double() * m
        for blk in cond[0].net:
            h = r
            for lyr in blk.net.net:
                h = torch.nn.functional.linear(h, lyr.weight.double(), lyr.bias.double()) if isinstance(lyr, torch.nn.Linear) else lyr(h)
            r = r + h
        ls, sh = torch.nn.functional.linear(r, cond[1].weight.double(), cond[1].bias.double()).chunk(2, -1)
        want = (x.double() * ls.exp() + sh) * (1 - m) + x.double() * m
        layer = layer.to(DEV)
        y, ldj = layer.forward_and_log_det_jacobian(x.to(DEV))
        close(y, want.float(), atol=2e-5)
        close(ldj, (ls * (1 - m)).sum(-1, keepdim=True).float(), atol=2e-5)
        close(layer.inverse(y), x, atol=5e-5)
