"""Differential-equation nets with a closed-form Jacobian diagonal (reference: stribor/net/diffeq_exact_trace.py:12-72): for
``ContinuousTransform(..., divergence='exact')``.

``DiffeqExactTrace(exclusive_net, dimwise_net)``: f_i = dimwise_net(t, x_i, h_i, latent) with h = exclusive_net(t, x) hollow, so
df_i/dx_i = d dimwise_net / d x_i at fixed h_i -- one pass for the divergence instead of one reverse pass per dimension.  The
general evaluation is ``net.FuncAndDiagJac`` (any two modules, any device, a graph).  ``DiffeqExactTraceMLP`` is the MLP instance
(two MADEs + a ``DiffeqMLP``); same constructors and ``state_dict`` keys as the reference (``exclusive_net.net1.net.0.{weight,bias,
mask}``, ``dimwise_net.net.net.0.weight``), construction order net1, net2, dimwise net.

``DiffeqExactTraceDeepSet`` is the set instance over (..., N, dim) (diffeq_exact_trace.py:75-101): exclusive net
``DiffeqZeroTraceDeepSet`` (keys ``exclusive_net.elementwise.net.<i>.{weight,bias,mask}``,
``exclusive_net.interaction.set_emb.net.net.<i>.{weight,bias}``), the same dimwise net; construction order MADE, set embedding,
dimwise net.  ``closed_form_set`` / ``kernel_image_set`` are its counterparts of the functions below, for ``sx_cnf_exact_set_flow``.

``DiffeqExactTraceAttention`` is the attention instance over (..., N, dim) (diffeq_exact_trace.py:104-130): exclusive net
``DiffeqZeroTraceAttention`` (keys ``exclusive_net.q.net.<i>.{weight,bias,mask}``, ``exclusive_net.{k,v}.net.<i>.{weight,bias}``,
``exclusive_net.proj.net.0.{weight,bias}``), the same dimwise net; construction order q, k, v, proj, dimwise net.
``closed_form_attn`` / ``kernel_image_attn`` are its counterparts of the functions below, for ``sx_cnf_exact_attn_flow``.  The class is
exported here and not by the package namespace ``stribor_amd.net``.

For the MLP instance this module also holds what ``sx_cnf_exact_flow`` consumes: ``kernel_image`` stages ``mask * weight`` and the
dimwise weights into the kernel's LDS image (include/stribor_hip.h), and ``closed_form`` is the same arithmetic as torch ops --
value and forward-mode tangent side by side, no autograd -- in any dtype (tests hold it to ``autograd.functional.jacobian``).
"""
from typing import List

import numpy as np
import torch
import torch.nn as nn

from ..util.flatten_params import flatten_params
from . import cover
from .cover import tiles as _tiles
from .diagjac import FuncAndDiagJac
from .diffeq import DiffeqMLP
from .diffeq_zero_trace import DiffeqZeroTraceAttention, DiffeqZeroTraceDeepSet, DiffeqZeroTraceMLP, ZeroTraceEquivariantEncoder
from .made import MADE, MaskedLinear
from .mlp import MLP

__all__ = ['DiffeqExactTrace', 'DiffeqExactTraceMLP', 'DiffeqExactTraceDeepSet', 'DiffeqExactTraceAttention']

MAX_DIM, MAX_DH, MAX_LATENT, MAX_HIDDEN = 16, 8, 64, 64          # sx_cnf_exact_flow's coverage (SX_CNF_EXACT_MAX_*)
MAX_SET_SIZE = 128                                               # sx_cnf_exact_set_flow's (SX_CNF_EXACT_SET_MAX_*: the four above too)
POOLINGS = {'sum': 0, 'mean': 1, 'max': 2}                       # SX_POOL_*
SET_EXCHANGE_FLOATS = 128 * 16                                   # the kernel's LDS exchange buffer, after the image
# sx_cnf_exact_attn_flow's coverage (SX_CNF_EXACT_ATTN_MAX_*; d_h, latent, hidden and the set size as above) and its exchange: the k and v
# areas of 128 rows x 36 floats and 128 set flags
ATTN_MAX_DIM, ATTN_MAX_EMBED, ATTN_MAX_QUERY_TILES, ATTN_HEADS = 8, 32, 4, (1, 2, 4)
ATTN_EXCHANGE_FLOATS = 2 * 128 * 36 + 128


class DiffeqExactTrace(nn.Module):
    """forward(t [1], x [..., D], latent [..., L] | None) -> (f, Jacobian diagonal), or f alone with return_log_det_jac=False."""

    def __init__(self, exclusive_net, dimwise_net, return_log_det_jac: bool = True, **kwargs):
        super().__init__()
        self.exclusive_net = exclusive_net
        self.dimwise_net = dimwise_net
        self.return_log_det_jac = return_log_det_jac

    def forward(self, t, x, latent=None, **kwargs):
        params = flatten_params(self.exclusive_net, self.dimwise_net)
        y, jac = FuncAndDiagJac.apply(self.exclusive_net, self.dimwise_net, t, x, latent, params)
        return (y, jac) if self.return_log_det_jac else y


class DiffeqExactTraceMLP(DiffeqExactTrace):
    """``DiffeqExactTraceMLP(dim, hidden_dims, dim, d_h, latent_dim)``: exclusive net DiffeqZeroTraceMLP(dim, hidden_dims, d_h * dim),
    dimwise net DiffeqMLP(d_h + latent_dim + 2, hidden_dims, 1) over the columns [t, x_i, h_i, latent]."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, d_h: int, latent_dim: int = 0, return_log_det_jac: bool = True,
                 **kwargs):
        exclusive_net = DiffeqZeroTraceMLP(in_dim, hidden_dims, d_h * out_dim, return_log_det_jac=False, return_per_dim=True)
        dimwise_net = DiffeqMLP(d_h + latent_dim + 2, hidden_dims, 1)
        super().__init__(exclusive_net, dimwise_net, return_log_det_jac)


class DiffeqExactTraceDeepSet(DiffeqExactTrace):
    """``DiffeqExactTraceDeepSet(dim, hidden_dims, dim, d_h, latent_dim, pooling)`` over sets (..., N, dim): exclusive net
    DiffeqZeroTraceDeepSet(dim, hidden_dims, d_h * dim, pooling), dimwise net DiffeqMLP(d_h + latent_dim + 2, hidden_dims, 1) over
    the columns [t, x_i[d], h_i[d], latent_i].  `mask` is not passed on (``DiffeqExactTrace.forward``), so every element counts.

    `pooling` reaches the exclusive net (the reference's constructor drops it and always pools by 'max': DESIGN.md 4.11)."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, d_h: int, latent_dim: int = 0, pooling: str = 'max',
                 return_log_det_jac: bool = True, **kwargs):
        exclusive_net = DiffeqZeroTraceDeepSet(in_dim, hidden_dims, d_h * out_dim, pooling=pooling, return_log_det_jac=False)
        dimwise_net = DiffeqMLP(d_h + latent_dim + 2, hidden_dims, 1)
        super().__init__(exclusive_net, dimwise_net, return_log_det_jac)


class DiffeqExactTraceAttention(DiffeqExactTrace):
    """``DiffeqExactTraceAttention(dim, hidden_dims, dim, d_h, latent_dim, n_heads)`` over sets (..., N, dim): exclusive net
    DiffeqZeroTraceAttention(dim, hidden_dims, d_h * dim, n_heads), dimwise net DiffeqMLP(d_h + latent_dim + 2, hidden_dims, 1) over
    the columns [t, x_i[d], h_i[d], latent_i].  `mask` is not passed on (``DiffeqExactTrace.forward``), so every element counts."""

    def __init__(self, in_dim: int, hidden_dims: List[int], out_dim: int, d_h: int, latent_dim: int = 0, n_heads: int = 1,
                 return_log_det_jac: bool = True, **kwargs):
        exclusive_net = DiffeqZeroTraceAttention(in_dim, hidden_dims, d_h * out_dim, n_heads, return_log_det_jac=False)
        dimwise_net = DiffeqMLP(d_h + latent_dim + 2, hidden_dims, 1)
        super().__init__(exclusive_net, dimwise_net, return_log_det_jac)


# ---- the MLP instance, layer by layer ---------------------------------------------------------------------------------------------
def _structure(net):
    """The layers of a DiffeqExactTraceMLP-shaped module -> dict, or None when it is not the plain instance: two MADEs without a final
    activation, a DiffeqMLP over a plain MLP without one, one activation name and the same hidden widths in all three."""
    if type(net.exclusive_net) is not DiffeqZeroTraceMLP or type(net.dimwise_net) is not DiffeqMLP or type(net.dimwise_net.net) is not MLP:
        return None
    mades = [net.exclusive_net.net1, net.exclusive_net.net2]
    mlp = net.dimwise_net.net
    if any(type(m) is not MADE or m.final_activation is not None for m in mades) or mlp._wrapped or mlp.final_activation_name is not None:
        return None
    act = mlp.activation_name
    stacks = [list(m.net) for m in mades] + [list(mlp.net)]
    for stack, kind in zip(stacks, (MaskedLinear, MaskedLinear, nn.Linear)):
        if len(stack) % 2 != 1 or any(not isinstance(l, kind) for l in stack[0::2]):
            return None
        if any(type(a) is not getattr(nn, act, None) for a in stack[1::2]):
            return None
    if any(m.activation != act for m in mades):
        return None
    lins = [stack[0::2] for stack in stacks]
    hidden = [l.out_features for l in lins[2][:-1]]
    if any([l.out_features for l in ls[:-1]] != hidden for ls in lins[:2]):
        return None
    D = lins[0][0].in_features
    if lins[1][0].in_features != D or lins[2][-1].out_features != 1:
        return None
    out = lins[0][-1].out_features
    if out % D or lins[1][-1].out_features != out:
        return None
    d_h = out // D
    L = lins[2][0].in_features - 2 - d_h
    if L < 0:
        return None
    return {'D': D, 'd_h': d_h, 'L': L, 'hidden': hidden, 'act': act, 'made': lins[:2], 'dimwise': lins[2],
            'activations': [a for stack in stacks for a in stack[1::2]]}


def _dimwise(s, t, x2, h, lat2, want_jac, cast, dtype):
    """The dimwise net of a structure dict on rows x2 [R, D] with h [R, D, d_h] and lat2 [R, L] | None -> (f [R, D], jac [R, D] | None):
    value and tangent d/dx_i side by side."""
    act, dact, _ = cover.ACTS[s['act']]
    d_h = s['d_h']
    dw = s['dimwise']
    W1, b1 = cast(dw[0].weight), cast(dw[0].bias)
    tt = (t.detach() if torch.is_tensor(t) else torch.tensor(float(t), dtype=torch.float64)).to(device=x2.device, dtype=dtype).reshape(())
    z = x2.unsqueeze(-1) * W1[:, 1] + h @ W1[:, 2:2 + d_h].t() + tt * W1[:, 0]
    if b1 is not None:
        z = z + b1
    if lat2 is not None:
        z = z + (lat2 @ W1[:, 2 + d_h:].t()).unsqueeze(-2)
    a = act(z)
    tau = dact(a) * W1[:, 1] if want_jac else None
    for l in dw[1:-1]:
        W, b = cast(l.weight), cast(l.bias)
        a_next = act(nn.functional.linear(a, W, b))
        if want_jac:
            tau = dact(a_next) * (tau @ W.t())
        a = a_next
    wl, bl = cast(dw[-1].weight)[0], cast(dw[-1].bias)
    f = a @ wl + (0 if bl is None else bl[0])
    return f, ((tau @ wl) if want_jac else None)


def closed_form(net, t, x, latent=None, want_jac: bool = True, dtype=None):
    """(f, jac) of a plain DiffeqExactTraceMLP by its closed form, as torch ops without autograd, in `dtype` (default: x's):
        h     = MADE_1(x) + MADE_2(x)                           (mask * weight)
        z_1   = W1[:, 0] t + W1[:, 1] x_i + W1[:, 2:2+d_h] h_i + W1[:, 2+d_h:] latent + b1,   tau_1 = act'(z_1) * W1[:, 1]
        z_l   = W_l act(z_{l-1}) + b_l,                                                       tau_l = act'(z_l) * (W_l tau_{l-1})
        f_i   = w_last . act(z_last) + b_last,                                                jac_i = w_last . tau_last
    (act' from the activation's OUTPUT, as the kernel takes it).  This is what sx_cnf_exact_flow evaluates per stage."""
    s = _structure(net)
    if s is None or s['act'] not in cover.ACTS or not s['hidden']:
        raise NotImplementedError('closed_form: a plain DiffeqExactTraceMLP with hidden layers and an activation of the kernel\'s set')
    act = cover.ACTS[s['act']][0]
    dtype = dtype or x.dtype
    D, d_h = s['D'], s['d_h']
    cast = lambda p: None if p is None else p.detach().to(device=x.device, dtype=dtype)
    x = x.detach().to(dtype)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, D)
    raw = 0
    for lins in s['made']:
        a = x2
        for i, l in enumerate(lins):
            a = nn.functional.linear(a, cast(l.mask) * cast(l.weight), cast(l.bias))
            if i + 1 < len(lins):
                a = act(a)
        raw = raw + a
    h = raw.reshape(-1, d_h, D).transpose(-1, -2)                     # [N, D, d_h]: column kk * D + i -> [i, kk]
    lat2 = None if latent is None else latent.detach().to(dtype).reshape(-1, latent.shape[-1])
    f, jac = _dimwise(s, t, x2, h, lat2, want_jac, cast, dtype)
    return f.reshape(*lead, D), (jac.reshape(*lead, D) if want_jac else None)


# ---- the kernel's LDS image -------------------------------------------------------------------------------------------------------
def _kmap(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def _out_tiles(d_h: int) -> int:
    return 1 if d_h <= 2 else 2 if d_h <= 4 else 4


_E = np.arange(1024)
_TILE_ROW = (_E >> 2) & 31
_TILE_COL = _kmap(4 * (_E >> 8) + (_E & 3), (_E >> 7) & 1)          # lane = (e >> 2) & 63, its upper half = bit 7 of e


def _fragment_image(Wp: np.ndarray) -> np.ndarray:
    """A zero-padded position-space matrix [32 MT, 32 KT] -> its MT x KT tiles of 1024 floats in A-fragment order."""
    MT, KT = Wp.shape[0] // 32, Wp.shape[1] // 32
    tiles = [Wp[32 * m + _TILE_ROW, 32 * c + _TILE_COL] for m in range(MT) for c in range(KT)]
    return np.concatenate(tiles).astype(np.float32)


def _covered(s, dim: int, latent_dim: int):
    """A structure dict (or None) -> itself when it is inside the ranges the two exact-trace kernels share, else None."""
    if s is None or s['D'] != dim or s['L'] != latent_dim:
        return None
    if not 1 <= dim <= MAX_DIM or not 1 <= s['d_h'] <= MAX_DH or latent_dim > MAX_LATENT:
        return None
    if len(s['hidden']) not in (1, 2) or any(not 1 <= w <= MAX_HIDDEN for w in s['hidden']):
        return None
    # the in-kernel activations and derivatives are those of torch's DEFAULT parameters
    return s if cover.kernel_activation(s['act'], s['activations']) else None


def kernel_coverage(net, dim: int, latent_dim: int):
    """The structure dict of `net` when sx_cnf_exact_flow covers it for rows of `dim` features and `latent_dim` latent columns, else
    None."""
    if type(net) is not DiffeqExactTraceMLP or not net.return_log_det_jac:
        return None
    return _covered(_structure(net), dim, latent_dim)


def kernel_tensors(s):
    """Every tensor the image is made of: the cache guards (weights, biases AND masks)."""
    ts = []
    for lins in s['made']:
        for l in lins:
            ts += [l.weight, l.mask] + ([] if l.bias is None else [l.bias])
    for l in s['dimwise']:
        ts += [l.weight] + ([] if l.bias is None else [l.bias])
    return ts


class _Image:
    """The parts of a kernel image in order, with the position tables and the blocks the two images share."""

    def __init__(self, s):
        D, d_h, hidden = s['D'], s['d_h'], s['hidden']
        self.d_h, self.L = d_h, s['L']
        self.HT, self.OT, self.NH = max(_tiles(w) for w in hidden), _out_tiles(d_h), len(hidden)
        self.pos_x = _kmap(np.arange(D), 0)
        cols = np.arange(d_h * D)
        self.pos_raw = 32 * ((cols // D) >> 1) + _kmap(cols % D, (cols // D) & 1)
        kk = np.arange(d_h)
        self.pos_e = _kmap(kk >> 1, kk & 1)                           # slot kk of the set embedding: register kk >> 1, lane half kk & 1
        self.pos_in = _kmap(1 + (kk >> 1), kk & 1)
        self.parts = []

    @staticmethod
    def npy(p):
        return p.detach().cpu().numpy().astype(np.float32)

    def vec(self, n_tiles, pos, values):
        v = np.zeros(32 * n_tiles, np.float32)
        if values is not None:
            v[pos] = values
        self.parts.append(v)

    def bias(self, n_tiles, pos, layer):
        self.vec(n_tiles, pos, None if layer.bias is None else self.npy(layer.bias))

    def mat(self, mt, kt, rpos, cpos, W):
        Wp = np.zeros((32 * mt, 32 * kt), np.float32)
        Wp[np.ix_(rpos, cpos)] = W
        self.parts.append(_fragment_image(Wp))

    def stage_made(self, lins, out_pos=None, out_tiles=None):
        """A MADE: mask * weight and the bias per layer, the last layer at the MADE output's positions (`out_pos` in `out_tiles`
        tiles: another layout of the last layer than the d_h slots')."""
        in_pos = self.pos_x
        pos_last, tiles_last = (self.pos_raw, self.OT) if out_pos is None else (out_pos, out_tiles)
        for i, l in enumerate(lins):
            last = i + 1 == len(lins)
            out_pos = pos_last if last else np.arange(l.out_features)
            mask = self.npy(l.mask)
            with np.errstate(invalid='ignore'):
                W = np.where(mask != 0, mask * self.npy(l.weight), np.float32(0))          # (0 * inf is not 0)
            self.mat(tiles_last if last else self.HT, 1 if i == 0 else self.HT, out_pos, in_pos, W)
            self.bias(tiles_last if last else self.HT, out_pos, l)
            in_pos = out_pos

    def stage_mlp(self, lins, out_pos):
        """A plain MLP on the state (no time column): weight and bias per layer, the last layer's outputs at `out_pos` of one tile."""
        in_pos = self.pos_x
        for i, l in enumerate(lins):
            last = i + 1 == len(lins)
            pos = out_pos if last else np.arange(l.out_features)
            self.mat(1 if last else self.HT, 1 if i == 0 else self.HT, pos, in_pos, self.npy(l.weight))
            self.bias(1 if last else self.HT, pos, l)
            in_pos = pos

    def stage_dimwise(self, dw):
        """The dimwise net's block, which ends both images -> (image, w_latent)."""
        HT, d_h = self.HT, self.d_h
        W1 = self.npy(dw[0].weight)
        h1 = np.arange(W1.shape[0])
        self.mat(HT, 1, h1, np.concatenate([[0], self.pos_in]), W1[:, 1:2 + d_h])
        self.bias(HT, h1, dw[0])
        self.vec(HT, h1, W1[:, 0])
        self.vec(HT, h1, W1[:, 1])
        if self.NH == 2:
            W2 = self.npy(dw[1].weight)
            self.mat(HT, HT, np.arange(W2.shape[0]), h1, W2)
            self.bias(HT, np.arange(W2.shape[0]), dw[1])
        wl = self.npy(dw[-1].weight)
        self.vec(HT, np.arange(wl.shape[1]), wl[0])
        self.bias(1, np.arange(1), dw[-1])
        return np.concatenate(self.parts), self.w_latent(W1)

    def w_latent(self, W1):
        """The latent columns of the dimwise first layer, zero-padded to whole tiles (None without latent columns)."""
        if not self.L:
            return None
        w = np.zeros((32 * self.HT, 32 * ((self.L + 31) // 32)), np.float32)
        w[:W1.shape[0], :self.L] = W1[:, 2 + self.d_h:]
        return w


def kernel_image(s):
    """-> (image [floats] fp32 numpy, w_latent [32 HT, 32 LT] fp32 numpy | None): the layout of include/stribor_hip.h
    (sx_cnf_exact_net).  The masks are multiplied in HERE: a weight entry under a zero mask never reaches the kernel."""
    im = _Image(s)
    for lins in s['made']:
        im.stage_made(lins)
    return im.stage_dimwise(s['dimwise'])


# ---- the set instance -------------------------------------------------------------------------------------------------------------
def _structure_set(net):
    """The layers of a DiffeqExactTraceDeepSet-shaped module -> dict, or None when it is not the plain instance: one MADE and two
    DiffeqMLPs over plain MLPs, none with a final activation, one activation name and the same hidden widths in all three."""
    ex = net.exclusive_net
    if type(ex) is not DiffeqZeroTraceDeepSet or type(ex.interaction) is not ZeroTraceEquivariantEncoder:
        return None
    made, emb, dim_net = ex.elementwise, ex.interaction.set_emb, net.dimwise_net
    if type(made) is not MADE or made.final_activation is not None or not made.return_per_dim:
        return None
    if any(type(m) is not DiffeqMLP or type(m.net) is not MLP or m.net._wrapped or m.net.final_activation_name is not None
           for m in (emb, dim_net)):
        return None
    act = dim_net.net.activation_name
    if made.activation != act or emb.net.activation_name != act or ex.interaction.pooling not in POOLINGS:
        return None
    stacks = [list(made.net), list(emb.net.net), list(dim_net.net.net)]
    for stack, kind in zip(stacks, (MaskedLinear, nn.Linear, nn.Linear)):
        if len(stack) % 2 != 1 or any(not isinstance(l, kind) for l in stack[0::2]):
            return None
        if any(type(a) is not getattr(nn, act, None) for a in stack[1::2]):
            return None
    lins = [stack[0::2] for stack in stacks]
    hidden = [l.out_features for l in lins[2][:-1]]
    if any([l.out_features for l in ls[:-1]] != hidden for ls in lins[:2]):
        return None
    D = lins[0][0].in_features
    out = lins[0][-1].out_features
    if out % D or lins[2][-1].out_features != 1 or ex.interaction.in_dim != D:
        return None
    d_h = out // D
    if lins[1][0].in_features != D + 1 or lins[1][-1].out_features != d_h:
        return None
    L = lins[2][0].in_features - 2 - d_h
    if L < 0:
        return None
    return {'D': D, 'd_h': d_h, 'L': L, 'hidden': hidden, 'act': act, 'pooling': ex.interaction.pooling, 'made': lins[0], 'emb': lins[1],
            'dimwise': lins[2], 'activations': [a for stack in stacks for a in stack[1::2]]}


def closed_form_set(net, t, x, latent=None, want_jac: bool = True, dtype=None):
    """(f, jac) of a plain DiffeqExactTraceDeepSet over sets x [..., N, D] (a 2-D x is one set) by its closed form, as torch ops
    without autograd, in `dtype` (default: x's):
        e_j   = set_emb([t, x_j])                               an MLP, d_h columns
        p_i   = pool over j != i of e_j                         'sum': (sum_j e_j) - e_i, the sum taken in element order;
                                                                'mean': that / max(N - 1, 1);  'max': N == 1 -> 0, else per column
                                                                e_i == first ? second : first (the two largest, duplicates count)
        h_i[d, :] = MADE(x_i)[d, :] + p_i                       (mask * weight)
    then the dimwise net with its tangent, as `closed_form`.  This is what sx_cnf_exact_set_flow evaluates per stage."""
    s = _structure_set(net)
    if s is None or s['act'] not in cover.ACTS or not s['hidden']:
        raise NotImplementedError('closed_form_set: a plain DiffeqExactTraceDeepSet with hidden layers and an activation of the kernel\'s set')
    act = cover.ACTS[s['act']][0]
    dtype = dtype or x.dtype
    D, d_h = s['D'], s['d_h']
    cast = lambda p: None if p is None else p.detach().to(device=x.device, dtype=dtype)
    x = x.detach().to(dtype)
    lead, N = x.shape[:-1], x.shape[-2]
    x2 = x.reshape(-1, D)
    a = x2
    for i, l in enumerate(s['made']):
        a = nn.functional.linear(a, cast(l.mask) * cast(l.weight), cast(l.bias))
        if i + 1 < len(s['made']):
            a = act(a)
    h = a.reshape(-1, d_h, D).transpose(-1, -2)                       # [R, D, d_h]: column kk * D + i -> [i, kk]
    tt = (t.detach() if torch.is_tensor(t) else torch.tensor(float(t), dtype=torch.float64)).to(device=x.device, dtype=dtype).reshape(())
    emb = s['emb']
    W1 = cast(emb[0].weight)
    e = x2 @ W1[:, 1:].t() + tt * W1[:, 0]
    if emb[0].bias is not None:
        e = e + cast(emb[0].bias)
    for l in emb[1:]:
        e = nn.functional.linear(act(e), cast(l.weight), cast(l.bias))
    e = e.reshape(-1, N, d_h)
    if N == 1:
        p = torch.zeros_like(e)
    elif s['pooling'] == 'max':
        first, second = torch.topk(e, 2, dim=-2).values.chunk(2, dim=-2)
        p = torch.where(e == first, second, first)
    else:
        tot = e[:, 0]
        for j in range(1, N):
            tot = tot + e[:, j]
        p = tot.unsqueeze(-2) - e
        if s['pooling'] == 'mean':
            p = p / max(N - 1, 1)
    h = h + p.reshape(-1, 1, d_h)
    lat2 = None if latent is None else latent.detach().to(dtype).expand(*lead, latent.shape[-1]).reshape(-1, latent.shape[-1])
    f, jac = _dimwise(s, t, x2, h, lat2, want_jac, cast, dtype)
    return f.reshape(*lead, D), (jac.reshape(*lead, D) if want_jac else None)


def kernel_coverage_set(net, dim: int, latent_dim: int, set_size: int):
    """The structure dict of `net` when sx_cnf_exact_set_flow covers it for sets of `set_size` elements of `dim` features and
    `latent_dim` latent columns, else None."""
    if type(net) is not DiffeqExactTraceDeepSet or not net.return_log_det_jac or not 1 <= set_size <= MAX_SET_SIZE:
        return None
    return _covered(_structure_set(net), dim, latent_dim)


def kernel_tensors_set(s):
    """Every tensor the image is made of: the cache guards (weights, biases AND the MADE's masks)."""
    ts = []
    for l in s['made']:
        ts += [l.weight, l.mask] + ([] if l.bias is None else [l.bias])
    for l in s['emb'] + s['dimwise']:
        ts += [l.weight] + ([] if l.bias is None else [l.bias])
    return ts


def kernel_image_set(s):
    """-> (image [floats] fp32 numpy, w_latent [32 HT, 32 LT] fp32 numpy | None): the layout of include/stribor_hip.h
    (sx_cnf_exact_set_net).  The masks are multiplied in HERE: a weight entry under a zero mask never reaches the kernel."""
    im = _Image(s)
    im.stage_made(s['made'])
    in_pos = im.pos_x
    for i, l in enumerate(s['emb']):
        last = i + 1 == len(s['emb'])
        out_pos = im.pos_e if last else np.arange(l.out_features)
        W = im.npy(l.weight)
        im.mat(1 if last else im.HT, 1 if i == 0 else im.HT, out_pos, in_pos, W[:, 1:] if i == 0 else W)
        im.bias(1 if last else im.HT, out_pos, l)
        if i == 0:
            im.vec(im.HT, out_pos, W[:, 0])
        in_pos = out_pos
    return im.stage_dimwise(s['dimwise'])


# ---- the attention instance -------------------------------------------------------------------------------------------------------
def _structure_attn(net):
    """The layers of a DiffeqExactTraceAttention-shaped module -> dict, or None when it is not the plain instance: a MADE q, plain MLPs
    k, v and a one-Linear proj, a DiffeqMLP over a plain MLP, none with a final activation, one activation name, hidden widths
    hidden[:-1] in q, k, v and E = hidden[-1] their output width."""
    ex, dim_net = net.exclusive_net, net.dimwise_net
    if type(ex) is not DiffeqZeroTraceAttention or type(dim_net) is not DiffeqMLP:
        return None
    q, mlps = ex.q, (ex.k, ex.v, ex.proj, dim_net.net)
    if type(q) is not MADE or q.final_activation is not None or not q.return_per_dim:
        return None
    if any(type(m) is not MLP or m._wrapped or m.final_activation_name is not None for m in mlps):
        return None
    act = dim_net.net.activation_name
    if q.activation != act or any(m.activation_name != act for m in mlps[:2]):
        return None
    stacks = [list(q.net)] + [list(m.net) for m in mlps]
    for stack, kind in zip(stacks, (MaskedLinear, nn.Linear, nn.Linear, nn.Linear, nn.Linear)):
        if len(stack) % 2 != 1 or any(not isinstance(l, kind) for l in stack[0::2]):
            return None
        if any(type(a) is not getattr(nn, act, None) for a in stack[1::2]):
            return None
    lq, lk, lv, lp, ld = [stack[0::2] for stack in stacks]
    hidden = [l.out_features for l in ld[:-1]]
    if not hidden or len(lp) != 1 or any([l.out_features for l in ls[:-1]] != hidden[:-1] for ls in (lq, lk, lv)):
        return None
    D, E, d_h = lq[0].in_features, hidden[-1], lp[0].out_features
    if lq[-1].out_features != E * D or any(ls[0].in_features != D or ls[-1].out_features != E for ls in (lk, lv)):
        return None
    if lp[0].in_features != E or ld[-1].out_features != 1 or not isinstance(ex.n_heads, int) or ex.n_heads < 1 or E % ex.n_heads:
        return None
    L = ld[0].in_features - 2 - d_h
    if L < 0:
        return None
    return {'D': D, 'd_h': d_h, 'L': L, 'hidden': hidden, 'act': act, 'E': E, 'heads': ex.n_heads, 'q': lq, 'k': lk, 'v': lv, 'proj': lp[0],
            'dimwise': ld, 'activations': [a for stack in stacks for a in stack[1::2]]}


def closed_form_attn(net, t, x, latent=None, want_jac: bool = True, dtype=None):
    """(f, jac) of a plain DiffeqExactTraceAttention over sets x [..., N, D] (a 2-D x is one set) by its closed form, as torch ops
    without autograd, in `dtype` (default: x's), H heads of width dh = E / H:
        q_i[d, :] = MADE_q(x_i)[d, :]                           (mask * weight; column e * D + d)
        k_j = K(x_j),  v_j = V(x_j)
        s_ij  = dh^-1/2 q_i[d] . k_j per head, s_ii = -inf      p_i = softmax_j(s_ij), a row without keys (N = 1): zeros
        o_i[d] = sum_j p_ij v_j,   h_i[d, :] = P o_i[d] + b
    then the dimwise net with its tangent, as `closed_form`.  This is what sx_cnf_exact_attn_flow evaluates per stage."""
    s = _structure_attn(net)
    if s is None or s['act'] not in cover.ACTS:
        raise NotImplementedError('closed_form_attn: a plain DiffeqExactTraceAttention with an activation of the kernel\'s set')
    dtype = dtype or x.dtype
    return _attn_value(s, t, x.detach().to(dtype), None if latent is None else latent.detach().to(dtype), want_jac, dtype)


def _attn_exclusive(s, x, dtype):
    """The exclusive net of closed_form_attn on a structure dict: x [..., N, D] in `dtype`, not detached -> h [R, D, d_h]."""
    act = cover.ACTS[s['act']][0]
    D, E, H = s['D'], s['E'], s['heads']
    cast = lambda p: None if p is None else p.detach().to(device=x.device, dtype=dtype)
    N = x.shape[-2]
    x2 = x.reshape(-1, D)

    def stack(lins, masked=False):
        a = x2
        for i, l in enumerate(lins):
            a = nn.functional.linear(a, cast(l.mask) * cast(l.weight) if masked else cast(l.weight), cast(l.bias))
            if i + 1 < len(lins):
                a = act(a)
        return a
    q = stack(s['q'], True).reshape(-1, N, E, D).transpose(-1, -2).reshape(-1, N, D, H, E // H)          # column e * D + d -> [d, e]
    k, v = (stack(s[n]).reshape(-1, N, H, E // H) for n in ('k', 'v'))
    sc = torch.einsum('bidhe,bjhe->bhdij', q, k) * (1 / (E // H)) ** 0.5
    sc = sc.masked_fill(torch.eye(N, dtype=torch.bool, device=x.device), -float('inf'))
    m = sc.max(-1, keepdim=True).values
    ex = torch.exp(sc - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    tot = ex.sum(-1, keepdim=True)
    p = torch.where(tot > 0, ex / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(ex))
    o = torch.einsum('bhdij,bjhe->bidhe', p, v).reshape(-1, D, E)
    return nn.functional.linear(o, cast(s['proj'].weight), cast(s['proj'].bias))


def _attn_value(s, t, x, latent, want_jac, dtype):
    """closed_form_attn's arithmetic on a structure dict; x and latent in `dtype`, not detached (the tests differentiate it)."""
    D = s['D']
    cast = lambda p: None if p is None else p.detach().to(device=x.device, dtype=dtype)
    lead = x.shape[:-1]
    h = _attn_exclusive(s, x, dtype)
    lat2 = None if latent is None else latent.expand(*lead, latent.shape[-1]).reshape(-1, latent.shape[-1])
    f, jac = _dimwise(s, t, x.reshape(-1, D), h, lat2, want_jac, cast, dtype)
    return f.reshape(*lead, D), (jac.reshape(*lead, D) if want_jac else None)


def _attn_slot(E: int) -> int:
    """Positions a dimension's query takes in a 32-position tile: 8, 16 or 32, the smallest that holds E."""
    return 8 if E <= 8 else 16 if E <= 16 else 32


def attn_query_tiles(E: int, dim: int) -> int:
    """Tiles of the q MADE's output in the kernel's layout: 32 // slot dimensions a tile."""
    per = 32 // _attn_slot(E)
    return (dim + per - 1) // per


def kernel_coverage_attn(net, dim: int, latent_dim: int, set_size: int):
    """The structure dict of `net` when sx_cnf_exact_attn_flow covers it for sets of `set_size` elements of `dim` features and
    `latent_dim` latent columns, else None.  Beyond the exact-trace kernels' shared ranges: dim <= 8, E <= 32, E * dim <= 128 with at
    most four query tiles (slot(E) * dim <= 128), 1, 2 or 4 heads."""
    if type(net) is not DiffeqExactTraceAttention or not net.return_log_det_jac or not 1 <= set_size <= MAX_SET_SIZE:
        return None
    s = _covered(_structure_attn(net), dim, latent_dim)
    if s is None or dim > ATTN_MAX_DIM or s['E'] > ATTN_MAX_EMBED or s['heads'] not in ATTN_HEADS:
        return None
    return s if attn_query_tiles(s['E'], dim) <= ATTN_MAX_QUERY_TILES else None


def kernel_tensors_attn(s):
    """Every tensor the image is made of: the cache guards (weights, biases AND the q MADE's masks)."""
    ts = []
    for l in s['q']:
        ts += [l.weight, l.mask] + ([] if l.bias is None else [l.bias])
    for l in s['k'] + s['v'] + [s['proj']] + s['dimwise']:
        ts += [l.weight] + ([] if l.bias is None else [l.bias])
    return ts


def kernel_image_attn(s):
    """-> (image [floats] fp32 numpy, w_latent [32 HT, 32 LT] fp32 numpy | None): the layout of include/stribor_hip.h
    (sx_cnf_exact_attn_net).  The masks are multiplied in HERE: a weight entry under a zero mask never reaches the kernel."""
    im = _Image(s)
    D, E = s['D'], s['E']
    slot = _attn_slot(E)
    per = 32 // slot
    cols = np.arange(E * D)
    d, e = cols % D, cols // D
    im.stage_made(s['q'], 32 * (d // per) + (d % per) * slot + e, attn_query_tiles(E, D))
    im.stage_mlp(s['k'], np.arange(E))
    im.stage_mlp(s['v'], np.arange(E))
    im.mat(1, 1, im.pos_e, np.arange(E), im.npy(s['proj'].weight))
    im.bias(1, im.pos_e, s['proj'])
    return im.stage_dimwise(s['dimwise'])
