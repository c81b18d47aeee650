"""fp64 restatements for the IResNet / ContinuousIResNet training tests (tests/test_gpu_iresnet_train.py,
tests/test_iresnet_train_host.py): the product MLP with spectral norm, the forward map, the implicit backward of the fixed-point
inverse, and a context that sends a module down the composition path."""
import contextlib

import torch
import torch.nn as nn

import stribor_amd as st

ACTS64 = {'ReLU': torch.relu, 'Tanh': torch.tanh, 'Sigmoid': torch.sigmoid, 'SiLU': nn.functional.silu,
          'GELU': nn.functional.gelu, 'ELU': nn.functional.elu, 'Softplus': nn.functional.softplus,
          'LeakyReLU': nn.functional.leaky_relu, 'Hardtanh': nn.functional.hardtanh, None: lambda v: v}


class SinTime(nn.Module):
    """A time net the kernels do not know: evaluated by torch either way."""

    def __init__(self, dim):
        super().__init__()
        self.w = nn.Parameter(torch.randn(1, dim))

    def forward(self, t):
        return torch.sin(self.w * t) * t


# where a piecewise activation's derivative jumps
KINKS = {'ReLU': (0.0,), 'LeakyReLU': (0.0,), 'Hardtanh': (-1.0, 1.0)}


def kink_distance(f, net, x64):
    """The smallest distance of a hidden pre-activation of `net` at x64 from a kink of the module's activation (inf: it has none)."""
    pre = net.pre_activations(x64)[:-1]
    ks = KINKS.get(f.net.activation_name, ())
    return min([float('inf')] + [(a - k).abs().min().item() for a in pre for k in ks])


def linears(f):
    return [m for m in f.net.net if isinstance(m, nn.Linear)]


def weight_param(lin):
    return lin.weight_orig if hasattr(lin, 'weight_orig') else lin.weight


class Net64:
    """fp64 leaves of a module's tensors AS THEY ARE NOW: per layer W (weight_orig of a wrapped layer), b, u, v; the time net as an
    fp64 deep copy.  `advance(n_power)` runs the hook's power iteration on u, v, as a training-mode call does."""

    def __init__(self, f):
        import copy
        self.layers = []
        for lin in linears(f):
            W = weight_param(lin).detach().double().cpu().requires_grad_()
            b = lin.bias.detach().double().cpu().requires_grad_()
            wrapped = hasattr(lin, 'weight_orig')
            u = lin.weight_u.detach().double().cpu().clone() if wrapped else None
            v = lin.weight_v.detach().double().cpu().clone() if wrapped else None
            self.layers.append([W, b, u, v])
        self.act = ACTS64[f.net.activation_name]
        self.final = ACTS64[f.net.final_activation_name]
        tn = getattr(f, 'time_net', None)
        self.time = None if tn is None else copy.deepcopy(tn).double().cpu()

    def advance(self, n_power):
        with torch.no_grad():
            for L in self.layers:
                W, _, u, v = L
                if u is None:
                    continue
                for _ in range(n_power):
                    v = nn.functional.normalize(W.t().mv(u), dim=0, eps=1e-12)
                    u = nn.functional.normalize(W.mv(v), dim=0, eps=1e-12)
                L[2], L[3] = u, v

    def pre_activations(self, x):
        """[a_1 .. a_L] at x (for the distance of a piecewise activation's inputs from its kink)."""
        out, h = [], x
        for i, (W, b, u, v) in enumerate(self.layers):
            Wn = W if u is None else W / torch.dot(u, W.mv(v))
            a = nn.functional.linear(h, Wn, b)
            out.append(a)
            h = self.act(a) if i + 1 < len(self.layers) else self.final(a)
        return out

    def g(self, x):
        h = x
        for i, (W, b, u, v) in enumerate(self.layers):
            Wn = W if u is None else W / torch.dot(u, W.mv(v))
            h = nn.functional.linear(h, Wn, b)
            h = self.act(h) if i + 1 < len(self.layers) else self.final(h)
        return h

    def s(self, t, n):
        if self.time is None:
            return None
        return self.time(t).expand(n, self.layers[-1][0].shape[0])

    def residual(self, x, t):
        s = self.s(t, x.shape[0])
        g = self.g(x)
        return g if s is None else s * g

    def forward(self, x, t=None):
        return x + self.residual(x, t)

    def params(self):
        """[W, b per layer] + the time net's parameters."""
        out = [p for L in self.layers for p in L[:2]]
        return out + ([] if self.time is None else list(self.time.parameters()))

    def implicit_backward(self, xstar, t, gx, iterations):
        """The K-step iteration w <- gx - J_r(x*)^T w from w = gx at the fixed point x*, then the cotangents of t and the parameters at
        -w: (w, gt | None, [parameter gradients in params() order])."""
        xr = xstar.detach().clone().requires_grad_()
        tr = None if t is None else t.detach().clone().requires_grad_()
        r = self.residual(xr, tr)
        w = gx
        for _ in range(iterations):
            (jtw,) = torch.autograd.grad(r, xr, w, retain_graph=True)
            w = gx - jtw
        wanted = ([] if tr is None else [tr]) + self.params()
        got = [torch.zeros_like(p) if g is None else -g for p, g in zip(wanted, torch.autograd.grad(r, wanted, w, allow_unused=True))]
        gt = got.pop(0) if tr is not None else None
        return w, gt, got


def module_grads(f):
    """The module's gradients in Net64.params() order (None -> zeros)."""
    ps = []
    for lin in linears(f):
        ps += [weight_param(lin), lin.bias]
    tn = getattr(f, 'time_net', None)
    ps += [] if tn is None else list(tn.parameters())
    return [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for p in ps]


@contextlib.contextmanager
def composed(f):
    """Inside: every graph-building call of `f` (one module, or a container of IResNet layers) takes the composition path."""
    mods = [m for m in f.modules() if isinstance(m, (st.IResNet, st.ContinuousIResNet))]
    for m in mods:
        m._train_plan = lambda: None
    try:
        yield f
    finally:
        for m in mods:
            del m._train_plan


def warm(f, t=False, n=5, device='cuda'):
    """A few training-mode calls: the power iteration settles and sigma bounds the Lipschitz constant."""
    mode = f.training
    f.train(True)
    with torch.no_grad():
        for _ in range(n):
            x = torch.randn(16, f.dim, device=device)
            f(x, t=torch.rand(16, 1, device=device)) if t else f(x)
    f.train(mode)
    return f
