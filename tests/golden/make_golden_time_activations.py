#!/usr/bin/env python3
"""Capture the F24 golden vectors (stribor/flows/activations.py:125-196, flows/cumsum.py:94-142, net/resnet.py and a NeuralFlow that
mixes time couplings with the two time-dependent activations) from the UNMODIFIED reference.

The recipe of make_golden_base.py: annotation-only stub modules (``torchtyping``, ``torchdiffeq``) ahead of the reference on
``sys.path``, no bytecode written, the reference untouched.  The fixture holds data only.

    python tests/golden/make_golden_time_activations.py <path of the reference checkout>

f24_time_activations.npz:
  tanh/{x, t}, tanh/log<0|1>/{y, x_back, ldiag}        ContinuousTanh(log_time) on x = randn(13, 3, 5) * 3, t in [0, 5); x_back = inverse(y, t)
  act/{x, t_rand}, act/<tanh|sigmoid|relu>/T<1|2.5>/{y_zero, y_rand, y_100}   ContinuousActivation at t = 0, rand, 100
  column/x, column/c<0|2>/{cumsum, diff}                CumsumColumn / DiffColumn on [2, 6, 3]
  resnet/state/<k>, resnet/{x, y}                       net.ResNet(4, [7, 5], 3)
  flow/state/<k>, flow/{x, t, t0, y_t, y_t_t0}          NeuralFlow([coupling, ContinuousTanh, coupling, ContinuousActivation(torch.tanh)]) at
                                                        dim 6: y_t = forward(x, t) of the full flow, y_t_t0 = forward(x, t, t0) of the flow
                                                        WITHOUT its last layer (which has no inverse)
  meta                                                  seeds, state_dict key lists, the flow's description
"""
import json
import os
import sys
import tempfile
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))          # repo root: flowdesc lives in stribor_amd.util
REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('STRIBOR_REFERENCE', ''))


def import_reference():
    stub = tempfile.mkdtemp(prefix='stribor_f24_stubs_')
    for name, body in (('torchtyping', 'class TensorType:\n    def __class_getitem__(cls, item):\n        return cls\n'),
                       ('torchdiffeq', 'def odeint(*a, **k):\n    raise NotImplementedError\n\n\nodeint_adjoint = odeint\n')):
        os.makedirs(os.path.join(stub, name))
        with open(os.path.join(stub, name, '__init__.py'), 'w') as f:
            f.write(body)
    sys.path.insert(0, REF)
    sys.path.insert(0, stub)
    import stribor  # noqa
    assert stribor.__file__.startswith(REF), stribor.__file__
    return stribor


ref = import_reference()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stribor_amd.util import flowdesc as fd  # noqa: E402

SEED = 2400
ACTS = {'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu}
COUPLINGS = [{'kind': 'continuous_affine_coupling', 'dim': 6, 'hidden': [13], 'mask': m, 'latent_dim': 0, 'time_kind': 'linear'}
             for m in ('ordered_left_half', 'ordered_right_half')]


def f24():
    arrays, meta = {}, {'seed': SEED, 'couplings': COUPLINGS}
    torch.manual_seed(SEED)
    with torch.no_grad():
        x = torch.randn(13, 3, 5) * 3
        t = torch.rand(13, 3, 1) * 5
        arrays['tanh/x'], arrays['tanh/t'] = x, t
        for lt in (0, 1):
            f = ref.ContinuousTanh(log_time=bool(lt))
            y = f(x, t)
            arrays[f'tanh/log{lt}/y'], arrays[f'tanh/log{lt}/x_back'] = y, f.inverse(y, t)
            arrays[f'tanh/log{lt}/ldiag'] = f.log_diag_jacobian(x, y, t)
        meta['tanh_state_keys'] = list(ref.ContinuousTanh().state_dict())

        x = torch.randn(7, 4, 5) * 2
        tr = torch.rand(7, 4, 1) * 2
        arrays['act/x'], arrays['act/t_rand'] = x, tr
        for name, fn in ACTS.items():
            for temp in (1.0, 2.5):
                f = ref.ContinuousActivation(fn, temperature=temp)
                for tag, tt in (('zero', torch.zeros_like(tr)), ('rand', tr), ('100', torch.full_like(tr, 100.0))):
                    arrays[f'act/{name}/T{temp:g}/y_{tag}'] = f(x, tt)
        meta['act_state_keys'] = list(ref.ContinuousActivation(torch.tanh).state_dict())

        x = torch.randn(2, 6, 3)
        arrays['column/x'] = x
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for c in (0, 2):
                arrays[f'column/c{c}/cumsum'] = ref.CumsumColumn(c)(x)
                arrays[f'column/c{c}/diff'] = ref.DiffColumn(c)(x)

        torch.manual_seed(SEED + 1)
        net = ref.net.ResNet(4, [7, 5], 3)
        for k, v in net.state_dict().items():
            arrays[f'resnet/state/{k}'] = v.clone()
        meta['resnet_state_keys'] = list(net.state_dict())
        x = torch.randn(9, 4)
        arrays['resnet/x'], arrays['resnet/y'] = x, net(x)

        torch.manual_seed(SEED + 2)
        c0, c1 = (fd.build_transform(ref, d) for d in COUPLINGS)
        layers = [c0, ref.ContinuousTanh(), c1, ref.ContinuousActivation(torch.tanh)]
        nf = ref.NeuralFlow(layers)
        for k, v in nf.state_dict().items():
            arrays[f'flow/state/{k}'] = v.clone()
        meta['flow_state_keys'] = list(nf.state_dict())
        x = torch.randn(11, 3, 6)
        t, t0 = torch.rand(11, 3, 1) * 2, torch.rand(11, 3, 1) * 2
        arrays['flow/x'], arrays['flow/t'], arrays['flow/t0'] = x, t, t0
        arrays['flow/y_t'] = nf(x, t=t)
        arrays['flow/y_t_t0'] = ref.NeuralFlow(layers[:3])(x, t=t, t0=t0)

    arrays = {k: v.detach().cpu().numpy() for k, v in arrays.items()}
    for k, v in arrays.items():
        assert np.isfinite(v).all(), k
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'f24_time_activations.npz')
    np.savez_compressed(path, **arrays)
    print(f'f24_time_activations: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays')


if __name__ == '__main__':
    f24()
