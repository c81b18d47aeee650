"""Which kernel a ContinuousTransform call picks (`ContinuousTransform._choose`, host code: the planners read shapes and the library's
LDS sizes, so the device may be the CPU).  Every expected value is a literal recorded from the if / elif chain `_solve` had before
the dispatch table replaced it, by driving the public methods with the launches intercepted -- not from the table under test."""
import pytest
import torch

import stribor_amd as st

DIM = 3
N = st.net
NETS = {
    'mlp1': lambda L: N.DiffeqMLP(DIM + 1 + L, [16], DIM),
    'mlp2': lambda L: N.DiffeqMLP(DIM + 1 + L, [40, 24], DIM),                    # (wider than the training kernels' 32)
    'mlp33': lambda L: N.DiffeqMLP(DIM + 1 + L, [33], DIM),
    'deepset': lambda L: N.DiffeqDeepset(DIM + 1 + L, [16, 8], DIM),
    'attn': lambda L: N.DiffeqSelfAttention(DIM + 1 + L, [16, 8], DIM, n_heads=2),
    'exact_mlp': lambda L: N.DiffeqExactTraceMLP(DIM, [16], DIM, 2, latent_dim=L),
    'exact_set': lambda L: N.DiffeqExactTraceDeepSet(DIM, [16, 12], DIM, 2, latent_dim=L, pooling='mean'),
    'uncovered': lambda L: torch.nn.Linear(DIM, DIM),
    # one step outside each planner's range
    'mlp_hidden129': lambda L: N.DiffeqMLP(DIM + 1, [129], DIM),
    'mlp_elu2': lambda L: N.DiffeqMLP(DIM + 1, [16], DIM, activation=torch.nn.ELU(alpha=2.0)),
    'exact_mlp_dh9': lambda L: N.DiffeqExactTraceMLP(DIM, [16], DIM, 9),
    'exact_set_dh9': lambda L: N.DiffeqExactTraceDeepSet(DIM, [16], DIM, 9),
    'attn_3heads': lambda L: N.DiffeqSelfAttention(DIM + 1, [16, 32], DIM, n_heads=3),
}

# (net, latent, divergence, set_data, training, x.shape, mask, graph wanted) -> the route
ROWS = [
    # the dense tier: the exact divergence of a row-wise net, or none; 'approximate' in eval mode is the exact divergence
    ('mlp1', 0, 'compute', False, False, (5, 3), False, False, 'sx_cnf_flow'),
    ('mlp2', 2, 'compute', False, False, (2, 4, 3), False, False, 'sx_cnf_flow'),
    ('mlp1', 0, 'compute', False, True, (5, 3), False, False, 'sx_cnf_flow'),
    ('mlp1', 0, 'none', False, False, (5, 3), False, False, 'sx_cnf_flow'),
    ('mlp1', 0, 'none', True, True, (2, 4, 3), False, False, 'sx_cnf_flow'),
    ('mlp1', 0, 'approximate', False, False, (5, 3), False, False, 'sx_cnf_flow'),
    ('mlp33', 0, 'approximate', False, False, (5, 3), False, False, 'sx_cnf_flow'),
    ('mlp1', 0, 'compute', False, False, (5, 3), True, False, 'composed'),
    ('mlp1', 0, 'compute', False, False, (5, 3), False, True, 'composed'),
    ('mlp1', 0, 'compute', True, False, (2, 4, 3), False, False, 'composed'),
    ('mlp1', 0, 'compute_set', False, False, (2, 4, 3), False, False, 'composed'),
    ('mlp1', 0, 'exact', False, False, (5, 3), False, False, 'composed'),
    # the training tier: asked first, with or without a graph; a width it does not cover trains on the composition path
    ('mlp1', 0, 'approximate', False, True, (5, 3), False, False, 'train'),
    ('mlp1', 2, 'approximate', False, True, (2, 4, 3), False, True, 'train'),
    ('mlp1', 0, 'approximate', False, True, (5, 3), True, False, 'composed'),
    ('mlp1', 0, 'approximate', True, True, (2, 4, 3), False, False, 'composed'),
    ('mlp33', 0, 'approximate', False, True, (5, 3), False, False, 'composed'),
    ('mlp33', 0, 'approximate', False, True, (5, 3), False, True, 'composed'),
    ('mlp2', 0, 'approximate', False, True, (5, 3), False, False, 'composed'),
    # sets: under 'none' the dense planner declines a DiffeqDeepset and the set tier takes it (a 2-D x is one set)
    ('deepset', 0, 'none', False, False, (2, 4, 3), False, False, 'sx_cnf_set_flow'),
    ('deepset', 0, 'none', False, False, (5, 3), False, False, 'sx_cnf_set_flow'),
    ('deepset', 2, 'compute', True, False, (2, 4, 3), False, False, 'sx_cnf_set_flow'),
    ('deepset', 0, 'compute_set', False, False, (2, 4, 3), False, False, 'sx_cnf_set_flow'),
    ('deepset', 0, 'approximate', True, False, (2, 4, 3), False, False, 'sx_cnf_set_flow'),
    ('deepset', 0, 'approximate', True, True, (2, 4, 3), False, False, 'composed'),
    ('deepset', 0, 'compute', False, False, (2, 4, 3), False, False, 'composed'),
    ('deepset', 0, 'compute', True, False, (2, 4, 3), True, False, 'composed'),
    ('deepset', 0, 'compute', True, False, (2, 4, 3), False, True, 'composed'),
    ('deepset', 0, 'exact', True, False, (2, 4, 3), False, False, 'composed'),
    # attention: the dense and the set planners decline, the attention tier takes it
    ('attn', 0, 'none', False, False, (2, 4, 3), False, False, 'sx_cnf_attn_flow'),
    ('attn', 2, 'compute_set', True, False, (2, 4, 3), False, False, 'sx_cnf_attn_flow'),
    ('attn', 0, 'compute', True, True, (5, 3), False, False, 'sx_cnf_attn_flow'),
    ('attn', 0, 'compute', False, False, (2, 4, 3), False, False, 'composed'),
    ('attn', 0, 'compute_set', False, False, (2, 4, 3), True, False, 'composed'),
    # exact trace: rows, and sets whatever set_data says (one row of a 2-D x is a set of N = 1)
    ('exact_mlp', 0, 'exact', False, False, (5, 3), False, False, 'sx_cnf_exact_flow'),
    ('exact_mlp', 2, 'exact', False, True, (2, 4, 3), False, False, 'sx_cnf_exact_flow'),
    ('exact_mlp', 0, 'exact', True, False, (5, 3), False, False, 'composed'),
    ('exact_mlp', 0, 'exact', False, False, (5, 3), False, True, 'composed'),
    ('exact_mlp', 0, 'compute', False, False, (5, 3), False, False, 'composed'),
    ('exact_set', 0, 'exact', False, False, (1, 3), False, False, 'sx_cnf_exact_set_flow'),
    ('exact_set', 0, 'exact', False, False, (1, 3), True, False, 'composed'),
    ('exact_set', 2, 'exact', True, False, (2, 4, 3), False, False, 'sx_cnf_exact_set_flow'),
    ('exact_set', 0, 'exact', False, False, (2, 4, 3), False, True, 'composed'),
    ('exact_set', 0, 'none', False, False, (2, 4, 3), False, False, 'composed'),
    # a module no kernel covers, and one step outside each planner's range
    ('uncovered', 0, 'compute', False, False, (5, 3), False, False, 'composed'),
    ('uncovered', 0, 'none', True, False, (2, 4, 3), False, False, 'composed'),
    ('uncovered', 0, 'approximate', False, True, (5, 3), False, False, 'composed'),
    ('mlp_hidden129', 0, 'compute', False, False, (5, 3), False, False, 'composed'),
    ('mlp_elu2', 0, 'compute', False, False, (5, 3), False, False, 'composed'),
    ('mlp_elu2', 0, 'approximate', False, True, (5, 3), False, True, 'composed'),
    ('deepset', 0, 'compute', True, False, (2, 128, 3), False, False, 'sx_cnf_set_flow'),
    ('deepset', 0, 'compute', True, False, (2, 129, 3), False, False, 'composed'),
    ('attn', 0, 'compute_set', True, False, (2, 129, 3), False, False, 'composed'),
    ('attn_3heads', 0, 'compute_set', True, False, (2, 4, 3), False, False, 'composed'),
    ('exact_mlp_dh9', 0, 'exact', False, False, (5, 3), False, False, 'composed'),
    ('exact_set_dh9', 0, 'exact', False, False, (2, 4, 3), False, False, 'composed'),
    ('exact_set', 0, 'exact', False, False, (2, 129, 3), False, False, 'composed'),
]

_made = {}


def _transform(net, latent, divergence, set_data):
    key = (net, latent, divergence, set_data)
    if key not in _made:
        _made[key] = st.ContinuousTransform(DIM, net=NETS[net](latent), divergence=divergence, has_latent=latent > 0, solver='rk4',
                                            solver_options={'step_size': 0.25}, set_data=set_data)
    return _made[key]


@pytest.mark.parametrize('row', ROWS, ids=lambda r: '-'.join(str(v) for v in r[:8]))
def test_route(row):
    net, latent, divergence, set_data, training, shape, masked, graph, want = row
    f = _transform(net, latent, divergence, set_data).train(training)
    for want_ldj in (True, False):
        route, plan, trace = f._choose(torch.Size(shape), latent, masked, graph, want_ldj, torch.device('cpu'))
        assert route == want
        assert (plan is None) == (route == 'composed')
        assert trace == (want_ldj and divergence != 'none')
