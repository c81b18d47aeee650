"""Helpers of the 'dopri5_per_sample' tests: an fp64 oracle of the solver specification (DESIGN.md "CNF"), written from the
specification alone -- its own tableau as exact fractions, the divergence by reverse mode, one controller per row -- on the module's
own weights cast to double, and the tight fp64 solve that stands for the truth."""
from fractions import Fraction as Fr

import torch

B = [Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84), Fr(0)]
B_STAR = [Fr(5179, 57600), Fr(0), Fr(7571, 16695), Fr(393, 640), Fr(-92097, 339200), Fr(187, 2100), Fr(1, 40)]
A = [[], [Fr(1, 5)], [Fr(3, 40), Fr(9, 40)], [Fr(44, 45), Fr(-56, 15), Fr(32, 9)],
     [Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)],
     [Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)], B[:6]]
C = [Fr(0), Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1), Fr(1)]
E = [b - s for b, s in zip(B, B_STAR)]

TIGHT_STEPS = 2000
DECISIVE_RATIO = (0.8, 1.25)
DECISIVE_CLAMP = 0.005


def net64(module, graph=False):
    """The DiffeqMLP of `module` in fp64 on the CPU with one time PER ROW: f(t [n], x [n, dim], latent) -> [n, dim], and its
    parameters (leaves that require grad when `graph`), in the order of module.parameters()."""
    ws, params = [], []
    for l in module.odefunc.diffeq.net.net:
        if isinstance(l, torch.nn.Linear):
            W = l.weight.detach().cpu().double().requires_grad_(graph)
            b = None if l.bias is None else l.bias.detach().cpu().double().requires_grad_(graph)
            ws.append((W, b))
            params += [W] + ([] if b is None else [b])
        else:
            ws.append(l)

    def f(t, x, latent):
        h = torch.cat([t.unsqueeze(-1), x] + ([] if latent is None else [latent]), -1)
        for w in ws:
            h = torch.nn.functional.linear(h, w[0], w[1]) if isinstance(w, tuple) else w(h)
        return h
    return f, params


def _wsum(w, ks):
    acc = 0
    for wj, kj in zip(w, ks):
        if wj != 0:
            acc = acc + float(wj) * kj
    return acc


def oracle(module, x, latent=None, reverse=False, atol=None, rtol=None, first_step=None, max_num_steps=4096, want_trace=True, graph=False):
    """The specification in fp64, row by row (vectorised: every row has its own s, dt and counters) -> dict:
    y [n, dim], a [n] (NaN where the row failed), accepted / rejected / status [n], ratios and fracs [attempts, n] (per attempt the
    error ratio and dt / remaining before the clamp; NaN where the row made no such attempt), decisive [n] (bool), evals [n], and with
    `graph` x (the leaf) and params (net64's leaves): y and a then carry the graph of the accepted arithmetic, the step sizes and
    decisions being constants."""
    atol = module.atol if atol is None else atol
    rtol = module.rtol if rtol is None else rtol
    f, params = net64(module, graph)
    lat = None if latent is None else latent.detach().cpu().double()
    t0, t1 = (module.T, 0.0) if reverse else (0.0, module.T)
    sgn = -1.0 if t1 < t0 else 1.0
    T = abs(t1 - t0)
    x64 = x.detach().cpu().double().requires_grad_(graph)
    n, dim = x64.shape

    def aug(s, v):
        with torch.enable_grad():
            vv = v if graph else v.detach().requires_grad_(True)
            dv = f(t0 + sgn * s, vv, lat)
            if want_trace:
                div = sum(torch.autograd.grad(dv[:, i].sum(), vv, create_graph=graph, retain_graph=True)[0][:, i] for i in range(dim))
            else:
                div = torch.zeros(n, dtype=torch.float64)
        return (sgn * dv, sgn * div) if graph else (sgn * dv.detach(), sgn * div.detach())

    rms = lambda v: v.pow(2).mean(-1).sqrt()

    def norm(vx, va):
        return torch.maximum(rms(vx), va.abs()) if want_trace else rms(vx)

    y, a, s = x64, torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    k1, q1 = aug(s, y)
    with torch.no_grad():
        if first_step is not None:
            dt = torch.full((n,), float(first_step), dtype=torch.float64)
        else:
            scale = atol + rtol * y.abs()
            d0, d1 = rms(y / scale), norm(k1 / scale, q1 / atol)
            h0 = torch.where((d0 < 1e-5) | (d1 < 1e-5), torch.full_like(d0, 1e-6), 0.01 * d0 / d1)
            kp, qp = aug(h0, y + h0.unsqueeze(-1) * k1)
            d2 = norm((kp - k1) / scale, (qp - q1) / atol) / h0
            h1 = torch.where((d1 <= 1e-15) & (d2 <= 1e-15), torch.clamp(1e-3 * h0, min=1e-6), (0.01 / torch.maximum(d1, d2)).pow(0.2))
            dt = torch.minimum(100 * h0, h1)
    done = torch.zeros(n, dtype=torch.bool) | (not T > 0)
    att, acc_n, rej_n, status = (torch.zeros(n, dtype=torch.int64) for _ in range(4))
    ratios, fracs = [], []
    nan = torch.full((n,), float('nan'), dtype=torch.float64)
    while True:
        with torch.no_grad():
            rem = T - s
            last = dt >= rem
            h = torch.where(last, rem, dt)
            cap = ~done & (att >= max_num_steps)
            status, done = torch.where(cap, 1, status), done | cap
            under = ~done & (s + h == s)
            status, done = torch.where(under, 2, status), done | under
            if bool(done.all()):
                break
            act = ~done
            fracs.append(torch.where(act, dt / rem, nan))
            h = torch.where(act, h, torch.zeros_like(h))
            att = att + act
        K, Q = [k1], [q1]
        for st in range(1, 7):
            ys = y + h.unsqueeze(-1) * _wsum(A[st], K)
            k, q = aug(s + float(C[st]) * h, ys)
            K.append(k)
            Q.append(q)
        y1, a1 = ys, a + h * _wsum(B, Q)
        with torch.no_grad():
            err_x, err_a = h.unsqueeze(-1) * _wsum(E, K), h * _wsum(E, Q)
            ratio = norm(err_x / (atol + rtol * torch.maximum(y.abs(), y1.abs())), err_a / (atol + rtol * torch.maximum(a.abs(), a1.abs())))
            ratios.append(torch.where(act, ratio, nan))
            finite = torch.isfinite(ratio)
            accept = act & finite & (ratio <= 1)
            floor = torch.where(ratio < 1, 1.0, 0.2).double()
            factor = torch.where(ratio == 0, torch.full_like(ratio, 10.0), torch.clamp(torch.maximum(0.9 * ratio.pow(-0.2), floor), max=10.0))
            s = torch.where(accept, torch.where(last, torch.full_like(s, T), s + h), s)
            acc_n, rej_n = acc_n + accept, rej_n + (act & ~accept)
            bad = act & ~finite
            status, done = torch.where(bad, 2, status), done | bad | (accept & last)
            dt = torch.where(act, h * factor, dt)
        y, a = torch.where(accept.unsqueeze(-1), y1, y), torch.where(accept, a1, a)
        k1, q1 = torch.where(accept.unsqueeze(-1), K[6], k1), torch.where(accept, Q[6], q1)
    failed = status != 0
    y, a = torch.where(failed.unsqueeze(-1), nan.unsqueeze(-1), y), torch.where(failed, nan, a)
    R = torch.stack(ratios) if ratios else torch.zeros(0, n, dtype=torch.float64)
    Fq = torch.stack(fracs) if fracs else torch.zeros(0, n, dtype=torch.float64)
    made = ~torch.isnan(Fq)
    lo, hi = DECISIVE_RATIO
    clear = ((R < lo) | (R > hi)) & ((Fq - 1).abs() > DECISIVE_CLAMP)
    decisive = (clear | ~made).all(0) & ~failed
    out = {'y': y, 'a': a, 'accepted': acc_n, 'rejected': rej_n, 'status': status, 'ratios': R, 'fracs': Fq, 'decisive': decisive,
           'evals': 6 * (acc_n + rej_n) + (1 if first_step is not None else 2)}
    if graph:
        out.update(x=x64, params=params)
    return out


def value_and_trace64(module, latent=None):
    """f(t, x) -> (dx/dt, tr d(dx/dt)/dx) of the module's DiffeqMLP in fp64 from the explicit Jacobian, layer by layer (J <- W J at a
    Linear, J <- act'(z) J at an activation, act' by reverse mode on the activation alone): the chain rule written out, which shares
    neither the kernel's collapsed constants nor the oracle's reverse passes, and costs no pass per feature."""
    dim = module.dim
    lat = None if latent is None else latent.detach().cpu().double()
    layers = [(l.weight.detach().cpu().double(), None if l.bias is None else l.bias.detach().cpu().double()) if isinstance(l, torch.nn.Linear) else l
              for l in module.odefunc.diffeq.net.net]

    def f(t, x):
        h = torch.cat([torch.full_like(x[:, :1], t), x] + ([] if lat is None else [lat]), -1)
        J = None
        for l in layers:
            if isinstance(l, tuple):
                J = l[0][:, 1:1 + dim].expand(x.shape[0], -1, -1) if J is None else l[0] @ J
                h = torch.nn.functional.linear(h, l[0], l[1])
            else:
                with torch.enable_grad():
                    z = h.detach().requires_grad_(True)
                    out = l(z)
                    d = torch.autograd.grad(out.sum(), z)[0]
                h, J = out.detach(), d.unsqueeze(-1) * J
        return h, J.diagonal(dim1=-2, dim2=-1).sum(-1)
    return f


def tight(module, x, latent=None, reverse=False):
    """The truth: rk4 (the 3/8 rule) on TIGHT_STEPS equal steps in fp64 -> (y [n, dim], log-det [n])."""
    f = value_and_trace64(module, latent)
    t0, t1 = (module.T, 0.0) if reverse else (0.0, module.T)
    dt = (t1 - t0) / TIGHT_STEPS
    y, l = x.detach().cpu().double(), torch.zeros(x.shape[0], dtype=torch.float64)
    for i in range(TIGHT_STEPS):
        t = t0 + i * dt
        k1, q1 = f(t, y)
        k2, q2 = f(t + dt / 3, y + dt * k1 / 3)
        k3, q3 = f(t + 2 * dt / 3, y + dt * (k2 - k1 / 3))
        k4, q4 = f(t + dt, y + dt * (k1 - k2 + k3))
        y, l = y + dt * (k1 + 3 * (k2 + k3) + k4) / 8, l + dt * (q1 + 3 * (q2 + q3) + q4) / 8
    return y, l


def units(y, l, ty, tl, atol, rtol):
    """Per row, the distance of (y, l) from the truth (ty, tl) in tolerance units, in the solver's own norm: max(rms over the row's
    entries of (y - ty) / (atol + rtol |ty|), |l - tl| / (atol + rtol |tl|)); NaN -> inf."""
    y, l = y.detach().cpu().double(), l.detach().cpu().double().reshape(-1)
    u = torch.maximum(((y - ty) / (atol + rtol * ty.abs())).pow(2).mean(-1).sqrt(), (l - tl).abs() / (atol + rtol * tl.abs()))
    return torch.where(torch.isnan(u), torch.full_like(u, float('inf')), u)


GAIN = 3.0          # every weight of a test net is scaled by it: at the default initialisation the dynamics are so mild that no step is rejected


def make(dim, hidden, act='Tanh', latent=0, seed=0, gain=GAIN, **kw):
    """A ContinuousTransform over a DiffeqMLP under 'dopri5_per_sample' in eval mode on the CPU; divergence 'compute' unless given."""
    import stribor_amd as st
    torch.manual_seed(seed)
    net = st.net.DiffeqMLP(dim + 1 + latent, hidden, dim, activation=act)
    with torch.no_grad():
        for lin in net.net.net:
            if isinstance(lin, torch.nn.Linear):
                lin.weight.mul_(gain)
    kw.setdefault('divergence', 'compute')
    kw.setdefault('solver', 'dopri5_per_sample')
    return st.ContinuousTransform(dim, net=net, has_latent=latent > 0, **kw).eval()
