"""CPU: the host-side planner (stribor_amd/fused.py, ProgramBuilder) plans every flow of a corpus exactly as the commit that wrote
tests/golden/plan_digests.json did -- sx_program bytes, blob sizes, column maps and every host-side table of every pack job.
Corpus, digest and fixture recipe: tests/golden/make_plan_digests.py."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_plan_digests as corpus  # noqa: E402

with open(corpus.FIXTURE) as _f:
    WANT = json.load(_f)


def test_corpus_and_fixture_hold_the_same_cases():
    """Every case has a fixture entry and the other way round; the entries without a digest ('raises' / null) are exactly the
    corpus's declared refusals, so no other case can pass without its digest being compared."""
    assert set(WANT) == set(corpus.CASES)
    assert {k for k, v in WANT.items() if not isinstance(v, dict)} == corpus.REFUSALS
    assert len(corpus.CASES) - len(corpus.REFUSALS) >= 140


@pytest.mark.parametrize('name', sorted(corpus.CASES))
def test_plan_digest(name):
    got, want = corpus.record(corpus.CASES[name]), WANT[name]
    if name in corpus.REFUSALS:
        assert got == want and want in ('raises', None), (got, want)
        return
    assert isinstance(got, dict), f'planned before, now {got!r}'
    assert got['kinds'] == want['kinds']              # first, in clear: where the step sequence diverged
    assert got['digest'] == want['digest']
