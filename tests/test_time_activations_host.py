"""Host (no GPU): the six names of the reference this package lacked -- ContinuousTanh, ContinuousActivation, CumsumColumn, DiffColumn,
net.ResNet, net.ResNetBlock -- their constructors, state_dict keys (fixture F24), what raises, and how a NeuralFlow that mixes time
couplings with the two time-dependent activations plans (step kinds of the one-launch program)."""
import inspect
import os
import re

import pytest
import torch

import stribor_amd as st
import timeacthelp as th
from stribor_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


def defaults(cls):
    return [(n, p.default) for n, p in inspect.signature(cls.__init__).parameters.items() if n not in ('self', 'kwargs')]


def test_names_and_constructor_signatures():
    E = inspect.Parameter.empty
    assert defaults(st.ContinuousTanh) == [('log_time', False)]
    assert defaults(st.ContinuousActivation) == [('activation', E), ('temperature', 1.0), ('learnable', False)]
    assert defaults(st.CumsumColumn) == [('column', E)] and defaults(st.DiffColumn) == [('column', E)]
    assert defaults(st.net.ResNetBlock) == [('dim', E), ('hidden_dims', E), ('activation', 'ReLU'), ('final_activation', None)]
    assert defaults(st.net.ResNet) == [('dim', E), ('hidden_dims', E), ('num_layers', E), ('activation', 'ReLU'), ('final_activation', None)]
    import stribor_amd.flows as flows
    for name in ('ContinuousTanh', 'ContinuousActivation', 'CumsumColumn', 'DiffColumn'):
        assert getattr(flows, name) is getattr(st, name)
    assert issubclass(st.ContinuousTanh, st.ElementwiseTransform) and issubclass(st.ContinuousActivation, st.ElementwiseTransform)
    assert issubclass(st.DiffColumn, st.CumsumColumn) and issubclass(st.CumsumColumn, st.Transform)


def test_state_dict_keys_equal_the_fixture():
    m = th.golden().meta
    assert list(st.ContinuousTanh().state_dict()) == m['tanh_state_keys'] == []
    f = st.ContinuousActivation(torch.tanh, temperature=2.5)
    assert list(f.state_dict()) == m['act_state_keys'] == ['temperature']
    assert isinstance(f.temperature, torch.nn.Parameter) and not f.temperature.requires_grad and f.temperature.item() == 2.5
    assert st.ContinuousActivation(torch.tanh, learnable=True).temperature.requires_grad
    assert list(st.ContinuousActivation(torch.nn.Tanh()).state_dict()) == ['temperature']
    net = st.net.ResNet(4, [7, 5], 3)
    assert list(net.state_dict()) == m['resnet_state_keys']
    assert all(re.fullmatch(r'net\.\d\.net\.net\.\d\.(weight|bias)', k) for k in net.state_dict())
    net.load_state_dict(th.golden().state('resnet'))
    nf, _ = th.mixed_flow(6)
    assert list(nf.state_dict()) == m['flow_state_keys']
    nf.load_state_dict(th.golden().state('flow'))


def test_what_raises_and_warns():
    f = st.ContinuousActivation(torch.tanh)
    x = torch.zeros(2, 3)
    with pytest.raises(NotImplementedError):
        f.inverse(x, t=x[..., :1])
    with pytest.raises(NotImplementedError):
        f.log_det_jacobian(x, x, t=x[..., :1])
    with pytest.raises(NotImplementedError):
        f.log_diag_jacobian(x, x, t=x[..., :1])
    for cls in (st.CumsumColumn, st.DiffColumn):
        with pytest.warns(RuntimeWarning, match='not tested'):
            assert cls(1).column == 1
    # the layer-wise autograd path of a NormalizingFlow takes ContinuousTanh (handing it `t`); ContinuousActivation has no log-det to
    # give that path and stays out of it (its own forward is differentiable: NeuralFlow trains through it)
    assert st.ContinuousTanh()._autograd_supported() and st.ContinuousTanh._autograd_takes_time and not f._autograd_supported()
    flow = st.NormalizingFlow(st.UnitNormal(3), [st.ContinuousTanh()])
    assert flow._layerwise_autograd_ok() and not st.NormalizingFlow(st.UnitNormal(3), [f])._layerwise_autograd_ok()
    t = torch.rand(4, 5, 1)
    assert flow._time_by_rows(t, (4, 5), CPU).shape == (20, 1) and flow._time_by_rows(t[:, :1], (4, 5), CPU).shape == (20, 1)
    assert flow._time_by_rows(torch.rand(4, 5, 3), (4, 5), CPU).shape == (20, 3) and flow._time_by_rows(1.5, (4, 5), CPU) == 1.5


def kinds(prog):
    return [prog.prog.steps[i].kind for i in range(prog.prog.n_steps)]


def test_mixed_neural_flow_plans_as_one_program():
    nf, _ = th.mixed_flow(6)
    prog = nf._fused(6, 0, False, CPU)
    assert prog is not None and kinds(prog) == [20, 25, 20, 25]
    s = prog.prog.steps
    assert (s[1].act, s[1].ldj_const, s[1].pad_) == (_hip.PWT_TANH_FLOW, 0.0, 0)
    assert (s[3].act, s[3].ldj_const, s[3].pad_) == (_hip.PWT_MIX_TANH, 1.0, 0)
    # ContinuousActivation has no inverse: with t0 the program is not built (layer by layer the reference's NotImplementedError leaves)
    assert nf._fused(6, 0, True, CPU) is None
    # without that layer: the mirrored inverse prefix at t0 (time slot 1, the inverse kind), then the forward pass at t
    nf3, _ = th.mixed_flow(6, last=False)
    prog = nf3._fused(6, 0, True, CPU)
    assert prog is not None and kinds(prog) == [20, 25, 20, 20, 25, 20]
    s = prog.prog.steps
    assert (s[1].act, s[1].pad_, s[1].reverse) == (_hip.PWT_TANH_FLOW_INV, 1, 0) and (s[4].act, s[4].pad_) == (_hip.PWT_TANH_FLOW, 0)
    assert [s[i].reverse for i in (0, 2, 3, 5)] == [1, 1, 0, 0]
    assert kinds(nf3._fused(6, 0, False, CPU)) == [20, 25, 20]
    # the step kinds alone form a program too; log_time and the temperature ride in the step
    solo = st.NeuralFlow([st.ContinuousTanh(log_time=True), st.ContinuousActivation(torch.nn.functional.relu, 2.5)])
    prog = solo._fused(33, 0, False, CPU)
    assert kinds(prog) == [25, 25] and prog.prog.steps[0].ldj_const == 1.0 and prog.prog.steps[1].ldj_const == 2.5
    assert prog.prog.steps[1].act == _hip.PWT_MIX_RELU
    # a latent input takes the tiles behind the data
    nfl, _ = th.mixed_flow(6, latent_dim=3)
    assert kinds(nfl._fused(6, 3, False, CPU)) == [20, 25, 20, 25]


def test_kernel_covered_callables_and_the_rest():
    F = torch.nn.functional
    cover = {_hip.PWT_MIX_TANH: (torch.tanh, F.tanh, torch.nn.Tanh()), _hip.PWT_MIX_SIGMOID: (torch.sigmoid, F.sigmoid, torch.nn.Sigmoid()),
             _hip.PWT_MIX_RELU: (torch.relu, F.relu, torch.nn.ReLU())}
    for kind, fns in cover.items():
        for fn in fns:
            assert st.ContinuousActivation(fn)._kind() == kind, fn

    class MyTanh(torch.nn.Tanh):
        pass
    for fn in (torch.sin, F.elu, lambda v: v, MyTanh(), torch.nn.ELU()):
        f = st.ContinuousActivation(fn)
        assert f._kind() is None
        assert st.NeuralFlow([st.ContinuousTanh(), f])._fused(6, 0, False, CPU) is None


def test_couplings_only_plan_as_before():
    descs = [th.coupling_desc(6, m) for m in ('ordered_left_half', 'ordered_right_half')]
    from stribor_amd.util import flowdesc as fd
    torch.manual_seed(0)
    nf = st.NeuralFlow([fd.build_transform(st, d) for d in descs])
    assert kinds(nf._fused(6, 0, False, CPU)) == [20, 20] and kinds(nf._fused(6, 0, True, CPU)) == [20, 20, 20, 20]
    assert st.NeuralFlow([])._fused(6, 0, False, CPU) is None


def test_temperature_guards_the_cached_program():
    nf, _ = th.mixed_flow(6)
    p1 = nf._fused(6, 0, False, CPU)
    assert nf._fused(6, 0, False, CPU) is p1
    with torch.no_grad():
        nf.transforms[3].temperature.fill_(2.5)
    p2 = nf._fused(6, 0, False, CPU)
    assert p2 is not p1 and p2.prog.steps[3].ldj_const == 2.5
    sd = {k: v.clone() for k, v in nf.state_dict().items()}
    sd['transforms.3.temperature'] = torch.tensor(0.5)
    nf.load_state_dict(sd)
    assert nf._fused(6, 0, False, CPU).prog.steps[3].ldj_const == 0.5


def test_new_step_and_mode_numbers():
    """SX_STEP_POINTWISE_TIME takes the next free number, the ABI version stays, and the programs that hold the step run kernel MODE 21
    from objects of their own (family 3), so that MODE 15's code object is what it was."""
    hdr = open(os.path.join(ROOT, 'include', 'stribor_hip.h')).read()
    steps = {n: int(v) for n, v in re.findall(r'#define (SX_STEP_\w+)\s+(\d+)', hdr)}
    assert steps['SX_STEP_POINTWISE_TIME'] == 25 == _hip.STEP_POINTWISE_TIME == max(steps.values())
    assert len(set(steps.values())) == len(steps) and steps['SX_STEP_COUPLING_TIME'] == 20 and steps['SX_STEP_MLP_INPUT'] == 24
    assert re.search(r'#define SX_ABI_VERSION 3\b', hdr)
    for name, v in re.findall(r'#define (SX_PWT_\w+) (\d+)', hdr):
        assert getattr(_hip, name[3:]) == int(v), name
    csrc = os.path.join(ROOT, 'stribor_amd', 'csrc')
    types = open(os.path.join(csrc, 'sx_flow_types.h')).read()
    assert '#define SX_MODE_TIME_POINTWISE 21' in types and re.search(r'#define SX_MODE_FAMILY\(MODE\) \(\(MODE\) == 21 \? 3 :', types)
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert '$(eval $(call FLOW_RULES,3))' in mk and 'sx_flow_x_$(p)_f3.o sx_flow_e_$(p)_f3.o' in mk and 'sx_pointwise_time.hip' in mk
    kernel = open(os.path.join(csrc, 'sx_flow_kernel.h')).read()
    assert 'SX_FM(SX_MODE_TIME_POINTWISE)' in kernel


def test_fixture_restatements_agree_with_the_reference():
    """The helper's literal restatements are what the fixture recorded from the reference, bit for bit on the CPU."""
    g = th.golden()
    x, t = g.t('tanh/x'), g.t('tanh/t')
    for lt in (0, 1):
        y = th.tanh_flow(x, t, bool(lt))
        assert torch.equal(y, g.t(f'tanh/log{lt}/y'))
        assert torch.equal(th.tanh_flow(y, t, bool(lt), True), g.t(f'tanh/log{lt}/x_back'))
        assert torch.equal(th.tanh_flow_ldiag(x, t, bool(lt)), g.t(f'tanh/log{lt}/ldiag'))
    x, tr = g.t('act/x'), g.t('act/t_rand')
    for name in th.ACTS:
        for temp in (1.0, 2.5):
            for tag, tt in (('zero', torch.zeros_like(tr)), ('rand', tr), ('100', torch.full_like(tr, 100.0))):
                assert torch.equal(th.mix(name, x, tt, torch.tensor(temp)), g.t(f'act/{name}/T{temp:g}/y_{tag}')), (name, temp, tag)
            assert torch.equal(g.t(f'act/{name}/T{temp:g}/y_zero'), x)
    # the mixed flow: the fixture's state through the restatement in fp32
    nf, descs = th.mixed_flow(6)
    state = g.state('flow')
    x, t, t0 = g.t('flow/x'), g.t('flow/t'), g.t('flow/t0')
    torch.testing.assert_close(th.mixed_flow_eval(descs, state, x, t, dtype=torch.float32), g.t('flow/y_t'), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(th.mixed_flow_eval(descs[:3], state, x, t, t0, dtype=torch.float32), g.t('flow/y_t_t0'), rtol=1e-5, atol=2e-5)
