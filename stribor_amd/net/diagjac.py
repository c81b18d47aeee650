"""f(x) and the diagonal of its Jacobian in one pass (reference: stribor/net/diagjac.py; Chen & Duvenaud, "Neural Networks with
Cheap Differential Operators", arXiv:1912.03579).

f_i = dimwise_net(t, x_i, h_i(, latent)) with h = exclusive_net(t, x) hollow (dh_i/dx_i = 0).  With h cut out of the graph, ONE
reverse pass of sum(f) with respect to x gives df_i/dx_i for every i.  The cut is repaired in the backward: the gradient that
arrives at the cut is sent on through the exclusive net, which yields the gradients of the un-cut composition.
"""
import torch

__all__ = ['FuncAndDiagJac']


def _flat_grads(grads, params):
    flat = [torch.zeros_like(p).view(-1) if g is None else g.contiguous().view(-1) for g, p in zip(grads, params)]
    return torch.cat(flat) if flat else torch.tensor([])


class FuncAndDiagJac(torch.autograd.Function):
    """``FuncAndDiagJac.apply(exclusive_net, dimwise_net, t, x, latent, flat_params[, order])`` -> (f [..., D], diag [..., D]).

    exclusive_net(t, x) -> [..., D * d_h], dimension-major; dimwise_net(t, x_i [B, 1], latent=[h_i, latent] [B, d_h + L]) -> [B, 1].
    t: [1]; latent: [..., L] or None; flat_params: ``util.flatten_params(exclusive_net, dimwise_net)`` -- the parameters reach
    autograd through it; order: the derivative taken of the diagonal (1: the Jacobian diagonal).  Both results are detached from the
    inner graph; the backward differentiates once."""

    @staticmethod
    def forward(ctx, exclusive_net, dimwise_net, t, x, latent, flat_params, order=1):
        ctx.nets = (exclusive_net, dimwise_net)
        with torch.enable_grad():
            t = t.detach().requires_grad_(True)
            x = x.detach().requires_grad_(True)
            if latent is not None:
                latent = latent.detach().requires_grad_(True)
            n_cols = x.numel()
            h = exclusive_net(t, x).reshape(n_cols, -1)
            h_cut = h.detach().requires_grad_(True)
            cond = h_cut
            if latent is not None:
                per_dim = latent.unsqueeze(-2).expand(*latent.shape[:-1], x.shape[-1], latent.shape[-1])
                cond = torch.cat([h_cut, per_dim.reshape(n_cols, -1)], -1)
            out = dimwise_net(t, x.reshape(n_cols, 1), latent=cond).reshape(x.shape)
            diag = torch.autograd.grad(out.sum(), x, create_graph=True)[0]
            for _ in range(order - 1):
                diag = torch.autograd.grad(diag.sum(), x, create_graph=True)[0]
        ctx.inner = (t, x, latent, h, h_cut, out, diag)
        return out.detach(), diag.detach()

    @staticmethod
    def backward(ctx, grad_out, grad_diag):
        t, x, latent, h, h_cut, out, diag = ctx.inner
        params = [p for net in ctx.nets for p in net.parameters()]
        live = [p for p in params if p.requires_grad]
        heads = [t, x, h_cut] + ([] if latent is None else [latent])
        outs, gouts = [out], [grad_out]
        if diag.requires_grad:                       # (a dimwise net that is affine in x has a constant diagonal)
            outs.append(diag)
            gouts.append(grad_diag)
        g = torch.autograd.grad(outs, heads + live, gouts, retain_graph=True, allow_unused=True)
        g_t, g_x, g_h = g[0], g[1], g[2]
        g_lat = None if latent is None else g[3]
        g_live = list(g[len(heads):])
        if g_h is not None and h.requires_grad:
            # through the cut: h's share of the gradients of x and of the parameters
            g2 = torch.autograd.grad(h, [x] + live, g_h, retain_graph=True, allow_unused=True)
            if g2[0] is not None:
                g_x = g2[0] if g_x is None else g_x + g2[0]
            g_live = [b if a is None else a if b is None else a + b for a, b in zip(g_live, g2[1:])]
        by_id = {id(p): gp for p, gp in zip(live, g_live)}
        g_flat = _flat_grads([by_id.get(id(p)) for p in params], params)
        return (None, None, g_t, g_x, g_lat, g_flat) + (None,) * (len(ctx.needs_input_grad) - 6)
