#!/usr/bin/env python3
"""Capture the F15 golden vectors (attention nets, stribor/net/attention.py:8-147) from the UNMODIFIED reference.

Same recipe as make_golden.py (annotation-only ``torchtyping`` / ``torchdiffeq`` stubs ahead of the reference on ``sys.path``,
no bytecode written, the reference untouched); run in the build container only.

    python tests/golden/make_golden_attention.py

No weights and no inputs are stored: every case builds its model under a seed (the init is held to the stored sha256 per tensor),
and then draws its inputs from the same RNG stream on the CPU, so a test rebuilds both with the product's host classes.

f15_attention.npz:
  grid/<model>/<shape>/h<n>/o<out>/H<heads>/d<diag>   test_attention.py:5-49: torch.manual_seed(123), the model
                    (n_points=11), x = randn(shape); y = model(x) (Attention: model(x, x, x)); mask = rand(shape[:-1], 1).round()
                    with mask[..., 0, 0] = 1, and y_mask = model(x, mask).  (The test's x_perm draw comes after these.)
  init/<model>/<in>/h<n>/o<out>   sha256 per state tensor of the grid's default init (heads / mask_diagonal do not change it)
  kernel/<model>/N<n>/H<heads>    kernel-sized sets: SelfAttention(4, [64], 3) (mask_diagonal when heads = 4) or
                    InducedSelfAttention(4, [64], 3, n_points = 16, or N when N = 33); x = randn(3, N, 4); y = model(x); mask:
                    set 0 all ones, set 1 values in {0, 0.5, 1} (element 0 = 1), set 2 all zeros; y_mask = model(x, mask).
  flow/<conditioner>      a 3-layer set flow of Coupling(Affine(4, latent_net=<conditioner>), set_data=True) (N = 16, latent 3):
                    x, latent = randn(8, 16, 4), randn(8, 16, 3); log_prob, forward, inverse; then the flow in float64:
                    grad/<param> of -log_prob(x, latent).mean().
"""
import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import import_reference  # noqa: E402,F401  (the stub recipe; importing it also imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flowdesc as fd  # noqa: E402

st = sys.modules['stribor']
torch.set_num_threads(8)

SHAPES = [(1, 1, 1), (10, 3, 2), (5, 3, 2, 3), (3, 2, 4, 6, 7)]
HIDDEN = [[32], [64, 32]]
OUTS = [1, 2, 5]
HEADS = [1, 4, 8]
MODELS = ['Attention', 'SelfAttention', 'InducedSelfAttention']
KERNEL_N = [1, 31, 33, 64, 257]


def npy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def sha(t):
    a = np.ascontiguousarray(npy(t))
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def grid_case(model, shp, hidden, out, heads, diag):
    return f'grid/{model}/{"x".join(map(str, shp))}/h{len(hidden)}/o{out}/H{heads}/d{int(diag)}'


def init_case(model, in_dim, hidden, out):
    return f'init/{model}/{in_dim}/h{len(hidden)}/o{out}'


def kernel_model(net, model, N, heads):
    if model == 'SelfAttention':
        return net.SelfAttention(4, [64], 3, n_heads=heads, mask_diagonal=heads == 4)
    return net.InducedSelfAttention(4, [64], 3, n_heads=heads, n_points=N if N == 33 else 16)


def kernel_mask(N):
    m = torch.ones(3, N, 1)
    m[1, :, 0] = torch.floor(torch.rand(N) * 3) / 2
    m[1, 0, 0] = 1
    m[2] = 0
    return m


def flow_desc(conditioner):
    masks = ['ordered_left_half', 'parity_even', 'ordered_right_half']
    hidden = [[32], [16, 32], [32]]
    extra = {'n_points': 5} if conditioner == 'induced_self_attention' else {}
    return [{'kind': 'coupling_affine', 'dim': 4, 'hidden': h, 'mask': m, 'latent_dim': 3, 'set_data': True,
             'net': conditioner, 'n_heads': 4, **extra} for m, h in zip(masks, hidden)]


def f15():
    arrays, meta = {}, {}
    for model in MODELS:
        for shp in SHAPES:
            for hidden in HIDDEN:
                for out in OUTS:
                    ic = init_case(model, shp[-1], hidden, out)
                    for heads in HEADS:
                        for diag in (True, False):
                            torch.manual_seed(123)                     # test_attention.py:13-18
                            m = getattr(st.net, model)(shp[-1], hidden, out, n_heads=heads, mask_diagonal=diag, n_points=11)
                            if ic not in meta:
                                meta[ic] = {'seed': 123, 'state_sha256': {k: sha(v) for k, v in m.state_dict().items()}}
                            x = torch.randn(*shp)
                            call = (lambda *a, **k: m(a[0], a[0], a[0], *a[1:], **k)) if model == 'Attention' else m
                            with torch.no_grad():
                                y = call(x)
                                mask = torch.rand(*shp[:-1], 1).round()   # test_attention.py:34-35
                                mask[..., 0, 0] = 1
                                y_mask = call(x, mask)
                            case = grid_case(model, shp, hidden, out, heads, diag)
                            arrays[f'{case}/y'], arrays[f'{case}/y_mask'] = y, y_mask
                            meta[case] = {'init': ic}
    for model in ('SelfAttention', 'InducedSelfAttention'):
        for N in KERNEL_N:
            for heads in (1, 4):
                case = f'kernel/{model}/N{N}/H{heads}'
                seed = 1500 + N + 7 * heads + (model == 'InducedSelfAttention')
                torch.manual_seed(seed)
                m = kernel_model(st.net, model, N, heads)
                hashes = {k: sha(v) for k, v in m.state_dict().items()}
                x = torch.randn(3, N, 4)
                mask = kernel_mask(N)
                with torch.no_grad():
                    arrays[f'{case}/y'], arrays[f'{case}/y_mask'] = m(x), m(x, mask)
                meta[case] = {'seed': seed, 'state_sha256': hashes}
    for cond in ('self_attention', 'induced_self_attention'):
        case = f'flow/{cond}'
        desc = flow_desc(cond)
        seed = 1515 + (cond == 'induced_self_attention')
        torch.manual_seed(seed)
        flow = fd.build_flow(st, desc, 4)
        hashes = {k: sha(v) for k, v in flow.state_dict().items()}
        x, latent = torch.randn(8, 16, 4), torch.randn(8, 16, 3)
        with torch.no_grad():
            arrays[f'{case}/log_prob'] = flow.log_prob(x, latent=latent)
            arrays[f'{case}/forward'] = flow.forward(x, latent=latent)
            arrays[f'{case}/inverse'] = flow.inverse(x, latent=latent)
        flow = flow.double()
        loss = -flow.log_prob(x.double(), latent=latent.double()).mean()
        loss.backward()
        arrays[f'{case}/loss64'] = loss.detach()
        for k, p in flow.named_parameters():
            arrays[f'{case}/grad/{k}'] = p.grad
        meta[case] = {'desc': desc, 'dim': 4, 'seed': seed, 'state_sha256': hashes}
    arrays = {k: npy(v) for k, v in arrays.items()}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'f15_attention.npz')
    np.savez_compressed(path, **arrays)
    print(f'f15_attention: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays')


if __name__ == '__main__':
    f15()
