"""Helpers of test_gpu_attention_core.py and of the oracle checks in test_attention_host.py: an fp64 restatement of the multi-head
attention of stribor/net/attention.py:26-49 that shares no code with the package, and the inputs of the sweep.

`oracle` is written from the formula, per head, out of place, so fp64 autograd through it gives the dq, dk and dv the backward
kernels are held to.  It calls neither torch.softmax nor anything of stribor_amd.

Every sweep case is four sets (leading dimension 4): set 0 unmasked (mask all ones), set 1 a random mask in {0, 0.5, 1} with key 0
live, set 2 a structured mask, set 3 fully masked.  The structured masks:
  'a'  the first ceil(Nk / 2) keys, rounded up to whole 32-key tiles when Nk > 32, are dead: the running max of the online softmax
       stays -inf over whole tiles and turns finite later;
  'b'  only the last key is live: nothing but the last (ragged) tile contributes.  Under mask_diagonal the last query then has no
       live key at all;
  'c'  only key 0 is live: under mask_diagonal query 0 loses its only key and must come out exactly 0 with a zero dq row.
"""
import functools
import math

import torch

import passhelp as ph
from cnfhelp import bound                  # noqa: F401  (8 x the fp32 reference's own error, floor 1e-6 * max(1, max |truth|))

N_SETS = 4

# (Nq = Nk, E, H, structured mask): each head width on one side of a HALF edge or an output-tile edge, each N a wave count
SWEEP = {
    'n32_dh8_half4_1wave': (32, 16, 2, 'a'),
    'n65_dh9_half8_3waves_ragged': (65, 9, 1, 'b'),
    'n96_dh17_half16_3waves': (96, 34, 2, 'c'),
    'n97_dh32_half16_4waves_ragged': (97, 32, 1, 'a'),
    'n70_dh33_half32_3waves': (70, 99, 3, 'b'),
    'n129_dh65_half64_2blocks': (129, 65, 1, 'c'),
    'n66_dh97_fourth_tile_1col': (66, 97, 1, 'a'),
    'n33_dh127_fourth_tile_ragged': (33, 127, 1, 'b'),
    'n96_dh128_widest': (96, 128, 1, 'c'),
    'n128_dh16_full_block': (128, 48, 3, 'a'),
}
# (Nq, Nk, E, H, structured mask): mask over the keys, no mask_diagonal, no output mask
CROSS = {
    'q65_k31_dh16': (65, 31, 64, 4, 'b'),
    'q5_k97_dh20': (5, 97, 40, 2, 'a'),
    'q96_k33_dh65': (96, 33, 130, 2, 'b'),
    'q1_k129_dh24': (1, 129, 24, 1, 'a'),
}
CASES = {**{k: (v[0],) + v for k, v in SWEEP.items()}, **CROSS}          # name -> (Nq, Nk, E, H, kind)

# large and shifted logits: (Nq = Nk, E, H) x variant
LOGIT_SHAPES = {'n65_dh33': (65, 33, 1), 'n96_dh128': (96, 128, 1)}
LOGIT_VARIANTS = ('x6', 'x12', 'x40', 'shift300', 'rising_tiles', 'falling_tiles')


def oracle(q, k, v, n_heads, mask_diagonal, mask):
    """(y [..., Nq, E], lse [..., H, Nq]) in fp64 on the CPU.  Per head: s = q k^T (1 / dh)^0.5; a key is live iff mask == 1 and,
    under mask_diagonal, key != query; weights exp(s - max over the live keys), 0 for dead keys, over their sum; a query without a
    live key gets y = 0 and lse = +inf; when Nq == Nk the rows of y are multiplied by the raw mask."""
    q, k, v = (t.to('cpu', torch.float64) for t in (q, k, v))
    Nq, E = q.shape[-2:]
    Nk = k.shape[-2]
    dh = E // n_heads
    live = torch.ones(*q.shape[:-2], Nq, Nk, dtype=torch.bool)
    if mask is not None:
        mask = mask.detach().to('cpu', torch.float64)
        live = live & (mask[..., 0] == 1).unsqueeze(-2)
    if mask_diagonal:
        live = live & ~torch.eye(Nq, Nk, dtype=torch.bool)
    has = live.any(-1, keepdim=True)
    ys, lses = [], []
    for h in range(n_heads):
        cols = slice(h * dh, (h + 1) * dh)
        s = torch.einsum('...id,...jd->...ij', q[..., cols], k[..., cols]) * (1 / dh) ** 0.5
        if Nk:
            top = torch.where(live, s, torch.full_like(s, -math.inf)).max(-1, keepdim=True).values.detach()
        else:
            top = torch.zeros(*s.shape[:-1], 1, dtype=torch.float64)
        top = torch.where(has, top, torch.zeros_like(top))
        w = torch.where(live, torch.exp(torch.where(live, s, top) - top), torch.zeros_like(s))
        z = torch.where(has, w.sum(-1, keepdim=True), torch.ones_like(top))
        ys.append(torch.einsum('...ij,...jd->...id', w / z, v[..., cols]))
        lses.append(torch.where(has, top + torch.log(z), torch.full_like(top, math.inf))[..., 0])
    y = torch.cat(ys, -1)
    if mask is not None and mask.shape[-2] == Nq:
        y = y * mask
    return y, torch.stack(lses, -2)


def structured_mask(kind, Nk):
    """[Nk] of 0 / 1 (module docstring)."""
    m = torch.zeros(Nk)
    if kind == 'a':
        dead = -(-Nk // 2)
        if Nk > 32:
            dead = -(-dead // 32) * 32
        assert 0 < dead < Nk
        m[dead:] = 1
    elif kind == 'b':
        m[Nk - 1] = 1
    else:
        assert kind == 'c'
        m[0] = 1
    return m


def random_mask(n_sets, Nk, g):
    """[n_sets, Nk, 1] in {0, 0.5, 1} with key 0 live."""
    m = torch.floor(torch.rand(n_sets, Nk, 1, generator=g) * 3) / 2
    m[:, 0] = 1
    return m


def sets_mask(kind, Nk, g):
    """[4, Nk, 1]: all ones, random, structured, all zeros."""
    m = torch.ones(N_SETS, Nk, 1)
    m[1] = random_mask(1, Nk, g)[0]
    m[2, :, 0] = structured_mask(kind, Nk)
    m[3] = 0
    return m


def _inputs(name, Nq, Nk, E):
    g = ph.generator(name)
    q = torch.randn(N_SETS, Nq, E, generator=g)
    k, v = (torch.randn(N_SETS, Nk, E, generator=g) for _ in range(2))
    gy = torch.randn(N_SETS, Nq, E, generator=g)
    return g, q, k, v, gy


@functools.lru_cache(maxsize=None)
def case(name):
    """The fp32 CPU inputs of a CASES entry: dict(q, k, v, gy, mask, n_heads, kind, cross).  Shared: do not modify."""
    Nq, Nk, E, H, kind = CASES[name]
    g, q, k, v, gy = _inputs(name, Nq, Nk, E)
    return dict(q=q, k=k, v=v, gy=gy, mask=sets_mask(kind, Nk, g), n_heads=H, kind=kind, cross=Nq != Nk)


def runs(name):
    """The (masked, mask_diagonal) runs of a case: with and without the mask, and mask_diagonal where Nq == Nk."""
    diags = (False,) if CASES[name][0] != CASES[name][1] else (False, True)
    return [(masked, diag) for masked in (False, True) for diag in diags]


def dead_queries(name, masked, diag):
    """[4, Nq] bool: the queries that have no live key BY CONSTRUCTION -- set 3 under the mask, and under the mask with
    mask_diagonal query 0 of mask 'c' and the last query of mask 'b' (the diagonal removes their only live key).  Every other
    query has a live key."""
    Nq, _, _, _, kind = CASES[name]
    dead = torch.zeros(N_SETS, Nq, dtype=torch.bool)
    if masked:
        dead[3] = True
        if diag and kind == 'c':
            dead[2, 0] = True
        if diag and kind == 'b':
            dead[2, Nq - 1] = True
    return dead


def truth_of(c, diag, mask):
    """dict(y, lse, dq, dk, dv): the oracle and its fp64 autograd on the inputs c (q, k, v, gy, n_heads) under `mask` (or None)."""
    q, k, v = (c[n].double().requires_grad_() for n in 'qkv')
    y, lse = oracle(q, k, v, c['n_heads'], diag, None if mask is None else mask.double())
    dq, dk, dv = torch.autograd.grad(y, (q, k, v), c['gy'].double())
    return dict(y=y.detach(), lse=lse.detach(), dq=dq, dk=dk, dv=dv)


@functools.lru_cache(maxsize=None)
def truth(name, masked, diag):
    """dict(y, lse, dq, dk, dv): the oracle and its fp64 autograd on case(name).  Shared: do not modify."""
    c = case(name)
    return truth_of(c, diag, c['mask'] if masked else None)


def live_counts(name, masked, diag):
    """[4, Nq] live keys per query (the same for every head)."""
    c = case(name)
    Nq, Nk = CASES[name][:2]
    live = torch.ones(N_SETS, Nq, Nk, dtype=torch.bool)
    if masked:
        live = live & (c['mask'][..., 0] == 1).unsqueeze(-2)
    if diag:
        live = live & ~torch.eye(Nq, Nk, dtype=torch.bool)
    return live.sum(-1)


def check_conditions(name):
    """The conditions on a sweep case that keep it from being trivial, asserted on the CPU and again before the GPU comparison:
    without mask_diagonal at least 90 % of the (head, query) rows of sets 0-2 see two live keys or more (set 2 of the masks 'b' and
    'c' is exempt: one live key by construction); the oracle's lse is +inf exactly at dead_queries; everything else is finite."""
    kind = CASES[name][4]
    sets = [0, 1] if kind in 'bc' else [0, 1, 2]
    n_live = live_counts(name, True, False)[sets]
    frac = (n_live >= 2).double().mean().item()
    assert frac >= 0.9, (name, frac)
    for masked, diag in runs(name):
        t = truth(name, masked, diag)
        dead = dead_queries(name, masked, diag)
        assert torch.equal(live_counts(name, masked, diag) == 0, dead), (name, masked, diag)
        inf = torch.isinf(t['lse']) & (t['lse'] > 0)
        assert torch.equal(inf, dead.unsqueeze(1).expand_as(inf)), (name, masked, diag)
        assert torch.isfinite(t['lse'][~inf]).all()
        for n in ('y', 'dq', 'dk', 'dv'):
            assert torch.isfinite(t[n]).all(), (name, masked, diag, n)


# ---- large and shifted logits ----------------------------------------------------------------------------------------------
def tile_maxima(q, k, n_heads):
    """[..., H, Nq, tiles]: the largest fp64 logit of each query within each 32-key tile."""
    Nq, E = q.shape[-2:]
    Nk = k.shape[-2]
    dh = E // n_heads
    qh = q.double().reshape(*q.shape[:-2], Nq, n_heads, dh)
    kh = k.double().reshape(*k.shape[:-2], Nk, n_heads, dh)
    s = torch.einsum('...ihd,...jhd->...hij', qh, kh) * (1 / dh) ** 0.5
    return torch.stack([s[..., j:j + 32].max(-1).values for j in range(0, Nk, 32)], -1)


@functools.lru_cache(maxsize=None)
def logit_case(shape, variant):
    """Inputs whose logits leave randn scale (dict as `case` plus shift = the vector added to k or None; mask = a random mask on
    every set).  Shared: do not modify.
      x6 / x12 / x40   q scaled: |logit| up to about 6, 12 and 40 times randn's;
      shift300         k + c for one vector c with c . q_i (1 / dh)^0.5 ~ N(0, 300^2): every logit of query i moves by the same
                       constant of order +-300, which the exact softmax does not see;
      rising_tiles     q and k share a direction u: logit_ij = noise_ij + 2 * tile(j) with |noise| well below 1, so each 32-key
                       tile's maximum exceeds the previous tile's for every query and the online softmax rescales at every tile.
                       The step is 2 and not tens: each earlier tile keeps a weight of order e^-2 in the result, so a wrong
                       rescale factor shows at its full size.  With steps beyond -log(fp32 eps) = 16.6 the earlier tiles vanish
                       from the fp32 result, y is a copy of the last tile's top value row and dq is 0 by cancellation: a
                       one-key softmax, which would pin nothing of the rescale's value;
      falling_tiles    the same keys (and values) in reverse order: the first tile holds the maximum, no rescale ever."""
    N, E, H = LOGIT_SHAPES[shape]
    g, q, k, v, gy = _inputs(f'{shape}/{variant}', N, N, E)
    dh = E // H
    shift = None
    if variant.startswith('x'):
        q = q * float(variant[1:])
    elif variant == 'shift300':
        u = torch.randn(E, generator=g)
        for h in range(H):
            u[h * dh:(h + 1) * dh] /= u[h * dh:(h + 1) * dh].norm()
        shift = 300.0 * dh ** 0.5 * u
        k = k + shift
    else:
        u = torch.randn(E, generator=g)
        for h in range(H):
            u[h * dh:(h + 1) * dh] /= u[h * dh:(h + 1) * dh].norm()
        tile = (torch.arange(N) // 32).to(torch.float32).reshape(1, N, 1)
        q = q + 2.0 * dh ** 0.5 * u
        k = 0.1 * k + 1.0 * tile * u
        if variant == 'falling_tiles':
            k, v = k.flip(-2).contiguous(), v.flip(-2).contiguous()
        else:
            assert variant == 'rising_tiles'
    return dict(q=q, k=k, v=v, gy=gy, mask=random_mask(N_SETS, N, g), n_heads=H, kind=None, cross=False, shift=shift)


@functools.lru_cache(maxsize=None)
def logit_truth(shape, variant, masked):
    c = logit_case(shape, variant)
    return truth_of(c, False, c['mask'] if masked else None)


def check_logit_conditions(shape, variant):
    """rising_tiles / falling_tiles: every query's tile maxima are strictly monotone (unmasked); shift300: the per-query shift is
    of order 300; every masked query keeps a live key (key 0)."""
    c = logit_case(shape, variant)
    if variant in ('rising_tiles', 'falling_tiles'):
        tm = tile_maxima(c['q'], c['k'], c['n_heads'])
        step = tm[..., 1:] - tm[..., :-1]
        assert tm.shape[-1] >= 3
        assert (step > 0).all() if variant == 'rising_tiles' else (step < 0).all(), (shape, variant)
    if variant == 'shift300':
        plain = c['k'].double() - c['shift'].double()
        moved = tile_maxima(c['q'], c['k'], c['n_heads']).max(-1).values - tile_maxima(c['q'], plain, c['n_heads']).max(-1).values
        assert 100 < moved.abs().median().item() < 400 and moved.abs().max().item() > 300, (shape, moved.abs().median().item())
    assert (c['mask'][:, 0, 0] == 1).all()

