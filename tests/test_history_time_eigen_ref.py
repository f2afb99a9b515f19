"""
CPU-only: the two routes of tests/history_time_eigen_ref.py against each other and against expected_history_eigen_ref.history.

The segment forms of pml_history_through_time_eigen (ls Phi(w t') rs with the two exponential factors; the two-factor lineage
posterior, q_p where t' = 0) give the numbers of the subdivided tree -- whole-branch sums only, no segment formula -- to what 60
digits leave, on the nine-tip tree of history_time_eigen_cases at k = 2, 4 and 20 (JTT) and M = 1, 3 and 7; the bins of boundaries
that cover the tree sum to history() of the original tree; a lineage row sums to the number of branches alive.

Both routes run with ``consistent``: Ainv is the inverse of the given A at 60 digits and the posteriors are the chain's own, since
two pieces of a branch compose to the whole branch only if Ainv A = 1 and the sweeps' top-down form needs pi_a P_ab = pi_b P_ba; on
the doubles numpy left the routes are two models 1e-16 apart (history_time_eigen_ref has the argument).

The measure is |a - b| / (the largest |entry| of that array for that bin).  AGREE is what was measured here: the worst ratio over
all cases is 1.39e-57 (k = 20, M = 7, tau = 0.011), so AGREE = 1e-55 has two digits to spare; the condition is that it stays
<= 1e-30, fourteen orders below what a double can show.  The sums against history() run on the given doubles, where they hold in
exact arithmetic whatever Ainv is, to the same bound; a lineage row of the given doubles sums to the number of branches alive to
what A Ainv differs from 1.
"""
import decimal

import numpy as np
import pytest

import expected_history_eigen_ref as eref
import history_time_eigen_cases as tcases
import history_time_eigen_ref as teref
import history_time_ref as tref
from f81_exact_ref import _CONTEXT, ZERO
from test_gpu_parity import random_spec

AGREE = decimal.Decimal('1e-55')
assert AGREE <= decimal.Decimal('1e-30')


def _spec(k):
    return tcases.jtt_spec() if k == 20 else random_spec('EIGEN', k, np.random.default_rng(40 + k))


def _gap(a, b):
    """The largest |x - y| over the largest |x| of two rows."""
    top = max(abs(x) for x in a)
    if top == 0:
        return ZERO if all(y == 0 for y in b) else decimal.Decimal('Infinity')
    return max(abs(x - y) for x, y in zip(a, b)) / top


def _compare(a, b, label):
    with decimal.localcontext(_CONTEXT):
        worst = ZERO
        for name in ('times', 'lineages'):
            for ra, rb in zip(a[name], b[name]):
                worst = max(worst, _gap(ra, rb))
        for ja, jb in zip(a['jumps'], b['jumps']):
            assert sorted(ja) == sorted(jb)
            rows = sorted(ja)
            worst = max(worst, _gap([x for i in rows for x in ja[i]], [x for i in rows for x in jb[i]]))
        worst = max(worst, _gap(a['bin_length'], b['bin_length']))
        print('routes {}: {:.3g}'.format(label, float(worst)))
        assert worst <= AGREE, (label, worst)


@pytest.mark.parametrize('M', [1, 3, 7])
@pytest.mark.parametrize('k', [2, 4, 20])
def test_segment_forms_give_the_subdivided_tree(k, M):
    flat, t, ids = tcases.nine_tips()
    masks = tcases.masks(flat, k, k)
    spec = _spec(k)
    bounds = tcases.boundaries(flat, t, ids, M)
    for sf, tau, tf in ((1.3, 0.0, 1.0), (0.8, 0.011, 0.95)):
        label = 'k={} M={} tau={}'.format(k, M, tau)
        sub = teref.by_subdivision(flat, masks, spec, t, bounds, sf, tau, tf, consistent=True)
        seg = teref.by_scaling(flat, masks, spec, t, bounds, sf, tau, tf, consistent=True)
        _compare(sub, seg, label)
        with decimal.localcontext(_CONTEXT):
            for row, count in zip(sub['lineages'], tref.crossing(flat.parent, t, bounds)):
                assert abs(sum(row, ZERO) - int(count)) <= AGREE * max(int(count), 1), label
        if M > 1:   # (a boundary crosses the branch of n1, which has t' = 0 at tau = 0 and an extent: its term is the root's posterior)
            assert ((bounds >= t[ids['root']]) & (bounds < t[ids['n1']])).any() and flat.dist[ids['n1']] == 0


@pytest.mark.parametrize('k', [2, 4, 20])
def test_bins_that_cover_the_tree_sum_to_the_whole_tree_history(k):
    """On the doubles as given: the segments of a branch tile its integral whatever Ainv is."""
    flat, t, ids = tcases.nine_tips()
    masks = tcases.masks(flat, k, k)
    spec = _spec(k)
    bounds = tcases.boundaries(flat, t, ids, 7)
    for sf, tau, tf in ((1.3, 0.0, 1.0), (0.8, 0.011, 0.95)):
        whole = eref.history(flat, masks, spec, sf, tau, tf)
        seg = teref.by_scaling(flat, masks, spec, t, bounds, sf, tau, tf)
        with decimal.localcontext(_CONTEXT):
            assert abs(sum(seg['bin_length'], ZERO) - whole['tree_length']) <= AGREE * whole['tree_length']
            assert _gap(whole['times'], [sum((row[s] for row in seg['times']), ZERO) for s in range(k)]) <= AGREE
            flat_whole = [x for i in range(k) for x in whole['jumps'][i]]
            flat_bins = [sum((jm[i][j] for jm in seg['jumps']), ZERO) for i in range(k) for j in range(k)]
            assert _gap(flat_whole, flat_bins) <= AGREE
            # a lineage row sums to the number of branches alive, to what A Ainv of the doubles differs from 1
            for row, count in zip(seg['lineages'], tref.crossing(flat.parent, t, bounds)):
                assert abs(float(sum(row, ZERO)) - int(count)) <= 1e-12 * max(int(count), 1)
