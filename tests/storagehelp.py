"""Helpers of the storage tests (tests/test_gpu_storage.py): the bf16 store criterion, the fp32 bound, and inputs whose base
pointer sits a few elements past a 16-byte boundary.

A kernel with bf16 storage computes in fp32 and rounds once, to nearest even, on the way out.  Against the fp64 value t of the
same operation such a store is off by at most half a bf16 ulp of t plus the fp32 arithmetic's own error, and the latter is held
to the project's measured tolerance (cnfhelp.bound: 8 x the CPU reference's own fp32 error, floored at 1e-6 * max(1, max |t|)).
A store that truncates, rounds ties away from zero or drops a low bit is a whole ulp off on a large share of the elements."""
import torch

from cnfhelp import bound

BF16_SUBNORMAL_SPACING = 2.0 ** -133      # 2^(1 - 127 - 7): the spacing of bf16 below its smallest normal 2^-126

WORST = {}                                # (launcher, 'f32' | 'bf16') -> largest err / bound seen in this process


def ulp_bf16(t64: torch.Tensor) -> torch.Tensor:
    """2^(floor(log2 |t|) - 7), floored at the subnormal spacing (frexp: |t| = m 2^e with m in [0.5, 1), exact at powers of two)."""
    a = t64.double().abs()
    _, e = torch.frexp(a)
    ulp = torch.ldexp(torch.ones_like(a), e - 8).clamp_min(BF16_SUBNORMAL_SPACING)
    return torch.where(a == 0, torch.full_like(a, BF16_SUBNORMAL_SPACING), ulp)


def _note(launcher, kind, ratio):
    if launcher is not None:
        WORST[(launcher, kind)] = max(WORST.get((launcher, kind), 0.0), ratio)


class Pool:
    """One bound per CASE.  A case of a dispatch table (branch x storage type x direction x output) is run at several row counts; its
    e_ref is the reference's own error over all of them, and so is max |t| of the floor.  (Launch by launch a one-row run of four
    columns would measure the reference on four numbers: there e_ref came out at 7e-8 for a log-det whose reference errors reach
    6e-6 over a few hundred elements -- a lucky draw, not the error of the fp32 sequence.)"""

    def __init__(self):
        self.e, self.m = {}, {}

    def add(self, key, ref32, truth64):
        if truth64.numel():
            t = truth64.detach().cpu().double()
            self.e[key] = max(self.e.get(key, 0.0), (ref32.detach().cpu().double() - t).abs().max().item())
            self.m[key] = max(self.m.get(key, 0.0), t.abs().max().item())

    def tol(self, key):
        """(tolerance, e_ref) by cnfhelp.bound's rule: 8 x e_ref, floored at 1e-6 * max(1, max |t|)"""
        e = self.e.get(key, 0.0)
        return max(8.0 * e, 1e-6 * max(1.0, self.m.get(key, 0.0))), e


def assert_bf16_store(got_bf16, ref32, truth64, what='', launcher=None, tol=None):
    """Every element: |float(got) - t| <= ulp_bf16(t) / 2 + cnfhelp.bound(ref32, truth64) (or the case's pooled bound `tol`).
    -> worst err / limit."""
    assert got_bf16.dtype == torch.bfloat16, got_bf16.dtype
    got = got_bf16.detach().cpu().double()
    ref32, t = ref32.detach().cpu(), truth64.detach().cpu().double()
    assert got.shape == t.shape == ref32.shape, (got.shape, ref32.shape, t.shape)
    if t.numel() == 0:
        return 0.0
    assert torch.isfinite(t).all() and torch.isfinite(got).all(), what
    tol, e_ref = bound(ref32, t) if tol is None else tol
    err = (got - t).abs()
    lim = 0.5 * ulp_bf16(t) + tol
    ratio = (err / lim).max().item()
    print(f'{what}: bf16 err {err.max().item():.3e} e_ref {e_ref:.3e} bound {tol:.3e} worst err/(ulp/2 + bound) {ratio:.3f}')
    _note(launcher, 'bf16', ratio)
    bad = err > lim
    if bad.any():
        i = (err - lim).argmax().item()
        raise AssertionError(f'{what}: {int(bad.sum())} of {t.numel()} bf16 elements beyond ulp/2 + {tol:.3e}: worst at {i}: got '
                             f'{got.flatten()[i].item():.9g}, fp64 {t.flatten()[i].item():.9g}, limit {lim.flatten()[i].item():.3e}')
    return ratio


def assert_f32(got, ref32, truth64, what='', launcher=None, tol=None):
    """max |got - t| <= cnfhelp.bound(ref32, truth64) (or the case's pooled bound `tol`) for an fp32 output.  -> err / bound."""
    assert got.dtype == torch.float32, got.dtype
    g = got.detach().cpu().double()
    ref32, t = ref32.detach().cpu(), truth64.detach().cpu().double()
    assert g.shape == t.shape == ref32.shape, (g.shape, ref32.shape, t.shape)
    if t.numel() == 0:
        return 0.0
    tol, e_ref = bound(ref32, t) if tol is None else tol
    err = (g - t).abs().max().item()
    print(f'{what}: fp32 err {err:.3e} e_ref {e_ref:.3e} bound {tol:.3e}')
    _note(launcher, 'f32', err / tol)
    assert err <= tol, (what, err, e_ref, tol)
    return err / tol


def assert_store(got, ref32, truth64, what='', launcher=None, tol=None):
    """The criterion of got's storage type."""
    return (assert_bf16_store if got.dtype == torch.bfloat16 else assert_f32)(got, ref32, truth64, what, launcher, tol)


def bits(t: torch.Tensor) -> torch.Tensor:
    """The elements' bit patterns (int16 / int32) on the CPU."""
    return t.detach().contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()


def offset_view(t: torch.Tensor, k: int) -> torch.Tensor:
    """t's values as a contiguous tensor whose data_ptr() is k elements past a 16-byte boundary, carved from a larger flat buffer
    (what a caller's `buf[1:1 + n * d].view(n, d)` or `xb[1:]` hands over: .contiguous() keeps such an offset)."""
    es = t.element_size()
    per16 = 16 // es
    buf = torch.empty(t.numel() + 2 * per16 + k, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % es == 0
    lead = (-(buf.data_ptr() // es)) % per16               # elements up to the next 16-byte boundary
    v = buf[lead + k: lead + k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (k * es) % 16
    return v
