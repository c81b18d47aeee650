#!/usr/bin/env python3
"""Capture the F14 golden vectors (IResNet / ContinuousIResNet, stribor/flows/iresnet.py) from the UNMODIFIED reference.

Same recipe as make_golden.py (annotation-only ``torchtyping`` / ``torchdiffeq`` stubs ahead of the reference on ``sys.path``,
no bytecode written, the reference untouched); run in the build container only.

    python tests/golden/make_golden_iresnet.py

f14_iresnet.npz:
  grid/<model>/<shape>/h<n>   test_resnet.py:23-64: shapes (10,2) (2,10) (1,10,2) (5,10,2), hidden [] / [32, 64]; IResNet (5 warm-up
                              calls) and ContinuousIResNet with TimeTanh / TimeFourierBounded(dim, hidden_dim=8), n_power_iterations=10
                              (10 warm-up calls).  State before the calls; then, in this order, y = f(x), x_back = f.inverse(y),
                              x_7 = f.inverse(y, iterations=7) in training mode with u / v / weight after each call; then y_eval,
                              x_back_eval in eval mode (and y_zero = f(x, t=0) for the continuous flows).
  neural_flow                 test_neural_flow.py:4-30, the full two-layer flow: y at t = 0, the t0 = t round trip, y for independent
                              t and t0, and the state after each call.
  seeds                       the default state of every grid case's seed, as sha256 per tensor (the init-stream check).
f14_iresnet_wide.npz:
  kernel/<dim>/<act>          dim 64 [64, 64] and dim 128 [128] at N = 256, ReLU (IResNet) and Tanh (ContinuousIResNet, TimeTanh):
                              state = the default init under the seed (sha256 per tensor); x, t regenerated from the seed on the
                              CPU; y, x_back and u / v after each call (training mode).
"""
import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference  # noqa: E402  (the stub recipe; importing it also imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flowdesc as fd  # noqa: E402

st = sys.modules['stribor']
torch.set_num_threads(8)

SHAPES = [(10, 2), (2, 10), (1, 10, 2), (5, 10, 2)]


def npy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def sha(t):
    a = np.ascontiguousarray(npy(t))
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def save(name, arrays, meta):
    arrays = {k: npy(v) for k, v in arrays.items()}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, name + '.npz')
    np.savez(path, **arrays)
    print(f'{name}: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays')


def sn_state(f, prefix=''):
    """u, v and the plain `weight` attribute of every spectral-normalised layer (the reference's hooks update them per call)."""
    out = {}
    for name, m in f.named_modules():
        if hasattr(m, 'weight_orig'):
            out[f'{prefix}{name}.weight_u'] = m.weight_u.clone()
            out[f'{prefix}{name}.weight_v'] = m.weight_v.clone()
            out[f'{prefix}{name}.weight'] = m.weight.detach().clone()
    return out


def grid_desc(model, dim, hidden):
    if model == 'iresnet':
        return {'kind': 'iresnet', 'dim': dim, 'hidden': hidden}
    return {'kind': 'continuous_iresnet', 'dim': dim, 'hidden': hidden, 'time_kind': model, 'time_hidden': 8,
            'n_power_iterations': 10}


def f14():
    arrays, meta = {}, {}
    seeds = {}
    for model in ('iresnet', 'tanh', 'fourier_bounded'):
        for shp in SHAPES:
            for hidden in ([], [32, 64]):
                dim = shp[-1]
                case = f'grid/{model}/{"x".join(map(str, shp))}/h{len(hidden)}'
                d = grid_desc(model, dim, hidden)
                cont = model != 'iresnet'
                torch.manual_seed(123)
                f = fd.build_transform(st, d)
                seeds[case] = {k: sha(v) for k, v in f.state_dict().items()}
                with torch.no_grad():
                    if cont:                                   # test_resnet.py:50-60
                        x = torch.randn(*shp)
                        t = torch.rand(*shp[:-1], 1) * 10
                        for _ in range(10):
                            f(x, t=t)
                    else:                                      # test_resnet.py:27-31
                        for _ in range(5):
                            x = torch.randn(*shp)
                            f(x)
                        t = None
                    x = torch.randn(*shp)
                    kw = {'t': t} if cont else {}
                    for k, v in f.state_dict().items():
                        arrays[f'{case}/state/{k}'] = v.clone()
                    arrays[f'{case}/x'] = x
                    if cont:
                        arrays[f'{case}/t'] = t
                    y = f(x, **kw)
                    for k, v in sn_state(f).items():
                        arrays[f'{case}/after_y/{k}'] = v
                    xb = f.inverse(y, **kw)
                    for k, v in sn_state(f).items():
                        arrays[f'{case}/after_x_back/{k}'] = v
                    x7 = f.inverse(y, iterations=7, **kw)
                    for k, v in sn_state(f).items():
                        arrays[f'{case}/after_x_7/{k}'] = v
                    f.eval()
                    ye = f(x, **kw)
                    xbe = f.inverse(ye, **kw)
                    arrays[f'{case}/y'], arrays[f'{case}/x_back'], arrays[f'{case}/x_7'] = y, xb, x7
                    arrays[f'{case}/y_eval'], arrays[f'{case}/x_back_eval'] = ye, xbe
                    if cont:
                        arrays[f'{case}/y_zero'] = f(x, t=torch.zeros_like(t))
                meta[case] = {'desc': d, 'shape': list(shp)}
    meta['seeds'] = {'seed': 123, 'state_sha256': seeds}

    # test_neural_flow.py:4-30: ContinuousAffineCoupling + ContinuousIResNet(dim, [32, 32], time_net=TimeTanh(dim))
    dim = 2
    desc = [{'kind': 'continuous_affine_coupling', 'dim': dim, 'hidden': [32], 'mask': 'ordered_0', 'latent_dim': 0,
             'time_kind': 'linear', 'time_out': dim, 'concatenate_time': False},
            {'kind': 'continuous_iresnet', 'dim': dim, 'hidden': [32, 32], 'time_kind': 'tanh'}]
    torch.manual_seed(123)
    nf = st.NeuralFlow([fd.build_transform(st, d) for d in desc])
    for k, v in nf.state_dict().items():
        arrays[f'neural_flow/state/{k}'] = v.clone()
    x = torch.randn(10, 4, 2)
    t = torch.zeros_like(x[..., :1])
    with torch.no_grad():
        arrays['neural_flow/x'] = x
        arrays['neural_flow/y_zero'] = nf(x, t=t)
        for k, v in sn_state(nf).items():
            arrays[f'neural_flow/after_y_zero/{k}'] = v
        t0 = torch.randn_like(x[..., :1])
        arrays['neural_flow/t0'] = t0
        arrays['neural_flow/y_round_trip'] = nf(x, t=t0, t0=t0)
        for k, v in sn_state(nf).items():
            arrays[f'neural_flow/after_y_round_trip/{k}'] = v
        t1 = torch.randn_like(x[..., :1])
        arrays['neural_flow/t1'] = t1
        arrays['neural_flow/y_t1_t0'] = nf(x, t=t1, t0=t0)
        for k, v in sn_state(nf).items():
            arrays[f'neural_flow/after_y_t1_t0/{k}'] = v
    meta['neural_flow'] = {'desc': desc, 'dim': dim}
    save('f14_iresnet', arrays, meta)

    # kernel-sized cases (kept in their own file: the rows dominate)
    arrays, meta = {}, {}
    for dim, hidden in ((64, [64, 64]), (128, [128])):
        for act in ('ReLU', 'Tanh'):
            case = f'kernel/{dim}/{act}'
            seed = 1400 + dim + (act == 'Tanh')
            d = ({'kind': 'iresnet', 'dim': dim, 'hidden': hidden, 'activation': act} if act == 'ReLU' else
                 {'kind': 'continuous_iresnet', 'dim': dim, 'hidden': hidden, 'activation': act, 'time_kind': 'tanh'})
            torch.manual_seed(seed)
            f = fd.build_transform(st, d)
            hashes = {k: sha(v) for k, v in f.state_dict().items()}
            torch.manual_seed(seed + 1)
            x = torch.randn(256, dim)
            t = torch.rand(256, 1)
            kw = {'t': t} if act == 'Tanh' else {}
            with torch.no_grad():
                y = f(x, **kw)
                for k, v in sn_state(f).items():
                    if not k.endswith('.weight'):
                        arrays[f'{case}/after_y/{k}'] = v
                xb = f.inverse(y, **kw)
                for k, v in sn_state(f).items():
                    if not k.endswith('.weight'):
                        arrays[f'{case}/after_x_back/{k}'] = v
            arrays[f'{case}/y'], arrays[f'{case}/x_back'] = y, xb
            meta[case] = {'desc': d, 'seed': seed, 'state_sha256': hashes}
    save('f14_iresnet_wide', arrays, meta)


if __name__ == '__main__':
    f14()
