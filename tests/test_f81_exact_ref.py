"""
CPU tests of tests/f81_exact_ref.py (the F81-family marginal pass in 60-digit decimal arithmetic): it agrees with the oracle and
with the real reference's golden values where float64 is a reference, and on the column blocks of
tests/test_gpu_optimiser_points.py the oracle itself stays inside the tolerance that test holds the device to.  Its joint
(max-product) sweep, joint_pass, against the oracle's joint sweep and against the enumeration of a small tree's assignments.
"""
import numpy as np
import pytest

import f81_exact_ref as exact
import optimiser_point_cases as cases
from conftest import load_golden, golden_forest, golden_spec
from oracle import pastml_oracle as orc

LNL_RTOL = 1e-11
POST_RTOL = 1e-9


@pytest.mark.parametrize('k', [2, 5, 20, 64])
def test_oracle_agrees_with_exact_values_away_from_small_tau(k):
    """sf avg in {1, 10} x tau in {0.02, avg}: no branch is shorter than 0.02 after the transform's shift, so 1 - e loses nothing
    and the oracle is held to the suite's own tolerances (ln L 1e-11, posteriors 1e-9)."""
    flat, stats = cases.forest()
    b = cases.build(k, 'F81')
    masks = cases.column_masks(b['batch'], 1, 1.0, None)
    pi = np.array(b['models'][1].frequencies)
    avg = stats.avg_nonzero_brlen
    for sf in (1 / avg, 10 / avg):
        for tau in (0.02, avg):
            tf = orc.tau_factor(tau, stats.forest_length, stats.num_nodes)
            want = exact.marginal_pass(flat, masks, pi, sf, tau, tf, top_down=True)
            got = orc.full_marginal_pass(flat, masks.astype(int), dict(kind=0, pi=pi), sf, tau, tf)
            np.testing.assert_allclose(got['loglik'], float(want['loglik']), rtol=LNL_RTOL)
            np.testing.assert_allclose(got['loglik_per_tree'], [float(x) for x in want['loglik_per_tree']], rtol=LNL_RTOL)
            np.testing.assert_allclose(got['posterior'], want['posterior'], rtol=POST_RTOL, atol=1e-300)
            with np.errstate(divide='ignore'):
                bu = np.log10(got['bu']) - got['bu_sf'][:, None]
                td = np.log10(got['td']) - got['td_sf'][:, None]
            for ours, theirs in ((bu, want['bu_log10']), (td, want['td_log10'])):
                assert np.array_equal(np.isinf(ours), np.isinf(theirs))
                fin = np.isfinite(theirs)
                np.testing.assert_allclose(ours[fin], theirs[fin], rtol=0, atol=1e-9)


def test_exact_value_of_the_reference_run_with_tau():
    """The real reference's ln L of Albania / Country under F81 with tau = 0.01 (golden) against the exact value."""
    z = load_golden('albania_F81')
    flat = golden_forest(z)
    spec, (sf, tau, tf) = golden_spec(z, 'tau_')
    assert tau > 0
    want = exact.marginal_pass(flat, z['tau_masks_initial'], spec['pi'], sf, tau, tf)
    np.testing.assert_allclose(float(z['tau_loglik']), float(want['loglik']), rtol=1e-11)
    assert exact.error_ratio(float(z['tau_loglik']), want, 1e-11) < 1


def test_pij_rows_sum_to_one_exactly():
    pi = np.random.default_rng(3).dirichlet(np.ones(5))
    for t in (0.0, 1e-11, 0.3, 40.):
        P, e = exact.pij(pi, t)
        with exact.decimal.localcontext(exact._CONTEXT):
            total = sum((exact.Decimal(float(x)) for x in pi), exact.ZERO)   # (one up to the rounding of pi itself)
            for row in P:
                assert abs(sum(row, exact.ZERO) - (1 - e) * total - e) < exact.Decimal(10) ** -55
        assert (e == 1) == (t == 0)


@pytest.mark.parametrize('k,family,shape', [c + ('random',) for c in cases.CASES] + [c + ('clumps',) for c in cases.CLUMP_CASES])
def test_oracle_stays_inside_the_tolerance_of_the_optimiser_point_tests(k, family, shape):
    """
    tol = LNL_RTOL |L| + 2^-53 G of tests/test_gpu_optimiser_points.py, asked of the oracle on that test's inputs (every point
    of every block, plain and tuple path alike): a float64 implementation whose exponential is within a unit of 2^-53 passes it.
    The worst ratio error / tol per regime of tau is printed (pytest -s).
    """
    b = cases.build(k, family, shape)
    flat, stats = b['flat'], b['stats']
    worst = {}
    for (c, sf0, tau0, kind), (pi, sf, tau, tf) in cases.all_blocks(b):
        for j in range(len(sf)):
            masks = cases.column_masks(b['batch'], c, tau[j], b['altered'][c])
            want = cases.exact_value(b, c, masks, pi[j], sf[j], tau[j], tf[j])
            got = orc.bottom_up(flat, masks.astype(int), dict(kind=0, pi=pi[j]), sf[j], tau[j], tf[j])['loglik']
            r = exact.error_ratio(got, want, LNL_RTOL)
            key = cases.regime(tau[j], stats.avg_nonzero_brlen)
            worst[key] = max(worst.get(key, 0.0), r)
    print('k = {} {} {}: worst error / tol of the oracle per regime of tau: {}'
          .format(k, family, shape, ', '.join('{} {:.3g}'.format(a, worst[a]) for a in sorted(worst))))
    assert max(worst.values()) < 1


@pytest.mark.parametrize('k', [2, 5, 20])
def test_oracle_joint_sweep_agrees_with_the_exact_joint_pass(k):
    """A benign random forest with three-child nodes, two trees and masks of every kind: the oracle's max-product ln L at 1e-11, its
    vectors at 1e-9 in log10 with the same zeros, every entry of its arg-max tables the exact first maximum or a maximum to 1e-12
    (choice_is_a_maximum), and the back-traced states those of the exact tables where no entry differs."""
    from pastml_amd.tree import FlatForest
    rng = np.random.default_rng(40 + k)
    flat = FlatForest.random(60, seed=k, max_arity=3, n_trees=2)
    pi = rng.dirichlet(np.ones(k) * 2)
    masks = np.ones((flat.n_nodes, k), dtype=int)
    for n in flat.tips:
        kind = rng.random()
        if kind < 0.8:
            masks[n] = 0
            masks[n, rng.integers(0, k, size=1 if kind < 0.7 else 2)] = 1
    rates = (1.7, 0.01, 0.95)
    want = exact.joint_pass(flat, masks, pi, *rates)
    got = orc.bottom_up(flat, masks, dict(kind=0, pi=pi), *rates, is_marginal=False)
    np.testing.assert_allclose(got['loglik'], float(want['loglik']), rtol=LNL_RTOL)
    with np.errstate(divide='ignore'):
        bu = np.log10(got['bu']) - got['bu_sf'][:, None]
    assert np.array_equal(np.isinf(bu), np.isinf(want['bu_log10']))
    fin = np.isfinite(bu)
    np.testing.assert_allclose(bu[fin], want['bu_log10'][fin], rtol=0, atol=1e-9)
    below = np.flatnonzero(flat.parent >= 0)
    differs = np.argwhere(got['joint_table'][below] != want['first_maximum'][below])
    for row, i in differs:
        n = int(below[row])
        assert exact.choice_is_a_maximum(want['products'], n, int(i), int(got['joint_table'][n, i])), (n, i)
    if not len(differs):
        states = orc.joint_backtrace(flat, got['bu'], got['joint_table'], pi)
        expect = np.zeros(flat.n_nodes, dtype=np.int64)
        for n in range(flat.n_nodes):
            p = int(flat.parent[n])
            expect[n] = want['root_first_maximum'][list(flat.roots).index(n)] if p < 0 else want['first_maximum'][n, expect[p]]
        assert np.array_equal(states, expect)


def test_exact_joint_pass_is_the_best_assignment_of_a_small_tree():
    """Three states, a tree of four tips (one ambiguous): the exact max-product likelihood is the largest probability over all 3^7
    assignments of states to nodes, enumerated in float64."""
    import itertools
    from pastml_amd.tree import FlatForest
    flat = FlatForest.balanced(2, seed=3)
    k = 3
    pi = np.array([0.5, 0.3, 0.2])
    masks = np.ones((flat.n_nodes, k), dtype=int)
    for n, allowed in zip(flat.tips, ([0], [2], [1, 2], [0])):
        masks[n] = 0
        masks[n, allowed] = 1
    want = exact.joint_pass(flat, masks, pi, 2.0)
    P = [np.array([[float(x) for x in row] for row in exact.pij(pi, t, 2.0)[0]]) for t in flat.dist]
    best = 0.0
    for states in itertools.product(range(k), repeat=flat.n_nodes):
        if all(masks[n, s] for n, s in enumerate(states)):
            p = pi[states[0]]
            for n in range(1, flat.n_nodes):
                p *= P[n][states[flat.parent[n]], states[n]]
            best = max(best, p)
    np.testing.assert_allclose(float(want['loglik']), np.log(best), rtol=1e-13)
