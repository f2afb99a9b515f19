"""
CPU-only: the two routes of tests/history_time_ref.py against each other and against expected_history_ref.history.

The partial-branch coefficients of pml_history_through_time (C0, C1a, C1b, Cee with A, B; the four-term lineage posterior) give
the numbers of the subdivided tree -- whole-branch sums only, no partial-branch formula -- to 1e-50 at 60 digits, on the inputs of
loglik_gradient_cases; and the bins of boundaries that cover the tree sum to history() of the original tree.

The frequencies are normalised as Decimals first.  Two pieces of a branch compose to the whole branch, P(t1) P(t2) = P(t1 + t2),
only if the frequencies sum to 1; doubles sum to 1 +- 1e-16, and with them the two routes -- two models that differ by that much
-- agree to 1e-16 and no further (the GPU tests' tolerance is five digits above it).
"""
import decimal

import numpy as np
import pytest

import expected_history_ref as href
import history_time_ref as tref
import loglik_gradient_cases as cases
from f81_exact_ref import _CONTEXT, ZERO
from pastml_amd.tree import FlatForest

AGREE = decimal.Decimal('1e-50')


def _frequencies(kind, k, seed):
    with decimal.localcontext(_CONTEXT):
        pi = [decimal.Decimal(float(x)) for x in cases.frequencies(kind, k, seed)]
        total = sum(pi, ZERO)
        return [x / total for x in pi]


def _close(x, y):
    return x == y or abs(x - y) <= AGREE * max(abs(x), abs(y))


def _compare(a, b, label):
    with decimal.localcontext(_CONTEXT):
        for name in ('times', 'lineages'):
            for m, (ra, rb) in enumerate(zip(a[name], b[name])):
                assert all(_close(x, y) for x, y in zip(ra, rb)), (label, name, m)
        for m, (ja, jb) in enumerate(zip(a['jumps'], b['jumps'])):
            assert sorted(ja) == sorted(jb)
            for i in ja:
                assert all(_close(x, y) for x, y in zip(ja[i], jb[i])), (label, 'jumps', m, i)
        assert all(_close(x, y) for x, y in zip(a['bin_length'], b['bin_length'])), (label, 'bin_length')


@pytest.mark.parametrize('shape', cases.SHAPES)
@pytest.mark.parametrize('kind, k', [('F81', 2), ('F81', 5), ('JC', 4)])
def test_coefficients_give_the_subdivided_tree(kind, k, shape):
    flat = cases.forest(shape, seed=k % 3)
    masks = cases.masks(flat, k, k)
    pi = _frequencies(kind, k, 1)
    t = tref.root_distance(flat)
    for tau in (0.0, 0.011):
        sf, tau, tf = cases.rates(k % 4, tau)
        label = '{} k={} {} tau={}'.format(kind, k, shape, tau)
        for bounds in (tref.covering_boundaries(t, 5), tref.covering_boundaries(t, 3)[1:3]):   # (the second: part of the tree)
            sub = tref.by_subdivision(flat, masks, pi, t, bounds, sf, tau, tf)
            coef = tref.by_coefficients(flat, masks, pi, t, bounds, sf, tau, tf)
            _compare(sub, coef, label)
            with decimal.localcontext(_CONTEXT):
                # a lineage row sums to the number of branches that cross its boundary
                for row, count in zip(sub['lineages'], tref.crossing(flat.parent, t, bounds)):
                    assert _close(sum(row, ZERO), decimal.Decimal(int(count))), label
        # the bins that cover the tree sum to the whole-tree history
        whole = href.history(flat, masks, pi, sf, tau, tf)
        sub = tref.by_subdivision(flat, masks, pi, t, tref.covering_boundaries(t, 5), sf, tau, tf)
        with decimal.localcontext(_CONTEXT):
            assert _close(sum(sub['bin_length'], ZERO), whole['tree_length']), label
            for s in range(k):
                assert _close(sum((row[s] for row in sub['times']), ZERO), whole['times'][s]), label
                for j in range(k):
                    assert _close(sum((jm[s][j] for jm in sub['jumps']), ZERO), whole['jumps'][s][j]), label


def test_slivers_long_branches_and_many_bins():
    """A boundary 1e-12 of a branch below its upper node, x = 800 cut in the middle, 200 bins on a 3-tip tree."""
    flat = cases.forest('ragged')
    k = 4
    masks = cases.masks(flat, k, 1)
    pi = _frequencies('F81', k, 2)
    mu = 1.0 / (1.0 - sum(float(x) ** 2 for x in pi))
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[::6]] = 800.0 / mu
    t = tref.root_distance(flat)
    n = int(branches[7])
    p = int(flat.parent[n])
    cut = t[p] + 1e-12 * (t[n] - t[p])
    long_one = int(branches[6])
    middle = 0.5 * (t[long_one] + t[int(flat.parent[long_one])])
    bounds = np.unique([t.min() - 1.0, cut, middle, t.max() + 1.0])
    _compare(tref.by_subdivision(flat, masks, pi, t, bounds), tref.by_coefficients(flat, masks, pi, t, bounds), 'slivers')
    small = FlatForest.random(3, seed=1, max_arity=2, zero_frac=0.0, n_trees=1)
    t = tref.root_distance(small)
    bounds = np.linspace(t.min(), t.max(), 201)
    masks = cases.masks(small, 3, 0)
    pi = _frequencies('F81', 3, 0)
    _compare(tref.by_subdivision(small, masks, pi, t, bounds), tref.by_coefficients(small, masks, pi, t, bounds), '200 bins')
