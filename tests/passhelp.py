"""Helpers of test_gpu_cnf_passes.py: batches large enough that every workgroup of a one-launch CNF kernel takes a second trip round
its pass loop, whatever grid the launcher picks.

The launcher (`cnf_launch`, sx_cnf_common.h) caps the grid at CUs x resident workgroups per CU and the grid is not visible from
Python.  A workgroup has 256 threads, so a CU holds at most max_threads_per_multi_processor // 256 of them (LDS and registers only
lower that): `cap_bound` is an upper bound of every grid, and a batch of 2.5 x cap_bound passes gives every workgroup at least two
trips and some workgroups one trip more than others.  A pass is 128 rows for the row kernels and (128 // N) * N rows for sets of N."""
import zlib

import torch

import stribor_amd as st

WG_THREADS = 256
WG_ROWS = 128
ROW_PERIOD = 77          # rows: coprime to 32 and 128
SET_PERIOD = 7           # sets: coprime to the 25, 3 and 1 sets per pass of set sizes 5, 33 and 128
ROW_TAIL = 45            # rows past a multiple of 128: wave 0 full, wave 1 partial, waves 2 and 3 empty
SET_TAIL = 2             # sets past a whole number of passes


def cap_bound(device):
    p = torch.cuda.get_device_properties(device)
    return p.multi_processor_count * (p.max_threads_per_multi_processor // WG_THREADS)


def passes_wanted(device):
    c = cap_bound(device)
    return 2 * c + c // 2


def rows_per_pass(set_size=1):
    return WG_ROWS if set_size == 1 else (WG_ROWS // set_size) * set_size


def n_passes(n_rows, set_size=1):
    return -(-n_rows // rows_per_pass(set_size))


def big_rows(device):
    """Rows of a big row-kernel batch: passes_wanted full passes and the ragged one."""
    return WG_ROWS * passes_wanted(device) + ROW_TAIL


def big_sets(device, set_size):
    """Sets of a big set-kernel batch: passes_wanted full passes and SET_TAIL sets more."""
    return (WG_ROWS // set_size) * passes_wanted(device) + SET_TAIL


def assert_multi_pass(n_rows, set_size, device):
    """The batch makes every workgroup take a second trip: its passes are at least 2.5 x the largest grid there can be."""
    have, need = n_passes(n_rows, set_size), passes_wanted(device)
    assert have >= need, (n_rows, set_size, have, need)
    return have


def seed_of(name):
    return zlib.crc32(name.encode())


def generator(name):
    return torch.Generator().manual_seed(seed_of(name))


def tile(t, n):
    """`t` repeated along its first axis and cut to n entries (entry i = t[i % len(t)])."""
    reps = -(-n // t.shape[0])
    return t.repeat(reps, *([1] * (t.dim() - 1)))[:n].contiguous()


def poison_outputs(monkeypatch, device):
    """torch.empty / empty_like hand out NaN-filled float tensors on the GPU for the rest of the test (the opt-in block of conftest.py,
    through the test's own monkeypatch): a row the kernel never wrote compares unequal instead of holding what the allocator returns."""
    e0, el0 = torch.empty, torch.empty_like

    def fill(t):
        return t.fill_(float('nan')) if t.is_floating_point() and t.is_cuda else t
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: fill(e0(*a, **k)))
    monkeypatch.setattr(torch, 'empty_like', lambda *a, **k: fill(el0(*a, **k)))
    probe = torch.empty(8, device=device)
    assert torch.isnan(probe).all() and torch.isnan(torch.empty_like(probe)).all()


def mismatch(big, small):
    """Rows of `big` that differ from `small[i % len(small)]` (both flattened to rows; NaN differs from everything) -> (count, first index)."""
    big, small = big.reshape(-1, big.shape[-1]), small.reshape(-1, small.shape[-1])
    period = small.shape[0]
    whole = big.shape[0] // period * period
    bad = (big[:whole].view(-1, period, big.shape[-1]) != small.unsqueeze(0)).any(-1).reshape(-1)
    tail = (big[whole:] != small[:big.shape[0] - whole]).any(-1)
    bad = torch.cat([bad, tail])
    n = int(bad.sum().item())
    return n, (int(bad.nonzero()[0].item()) if n else -1)


def assert_tiled(tag, big, small):
    """Every row i of `big` equals row i % period of `small`, bit for bit: torch.equal on the reshaped view plus the tail."""
    big, small = big.reshape(-1, big.shape[-1]), small.reshape(-1, small.shape[-1])
    period = small.shape[0]
    whole = big.shape[0] // period * period
    head = big[:whole].view(-1, period, big.shape[-1])
    ok = torch.equal(head, small.unsqueeze(0).expand_as(head)) and torch.equal(big[whole:], small[:big.shape[0] - whole])
    if not ok:
        n, first = mismatch(big, small)
        raise AssertionError(f'{tag}: {n} of {big.shape[0]} rows differ from the period\'s, the first at row {first}')


def max_error(big, truth64):
    """max |big[i] - truth64[i % period]| over every row of `big` (rows flattened; fp64 on big's device; NaN -> inf)."""
    big = big.reshape(-1, big.shape[-1]).double()
    t = truth64.reshape(-1, truth64.shape[-1]).to(big.device)
    period = t.shape[0]
    whole = big.shape[0] // period * period
    errs = [(big[:whole].view(-1, period, big.shape[-1]) - t.unsqueeze(0)).abs().reshape(-1), (big[whole:] - t[:big.shape[0] - whole]).abs().reshape(-1)]
    e = torch.cat(errs)
    return float('inf') if torch.isnan(e).any().item() else e.max().item()


def fp32_rows(f, x, lat=None, reverse=False):
    """A row-wise module's own composition path on the CPU in fp32: the reference's op sequence, whose error against the fp64
    restatement sets the bound (cnfhelp.bound)."""
    g = st.ContinuousTransform(f.dim, net=f.odefunc.diffeq, T=f.T, divergence=f.odefunc.divergence, has_latent=lat is not None,
                               solver=f.test_solver, solver_options=f.test_solver_options).eval()
    return g._composed_reference(x, lat, reverse=reverse)
