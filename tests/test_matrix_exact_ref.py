"""
CPU tests of tests/matrix_exact_ref.py (the marginal pass of the eigen models and HKY in 50-digit decimal arithmetic): the
restatement against closed cases, and the oracle held to the suite's tolerances against it on the inputs of
tests/test_gpu_eigen_shapes.py (tests/eigen_shape_cases.py) -- the condition under which those tolerances, asked of the device
against exact values, are meaningful: a float64 implementation of the reference's operation sequence passes them with two to
three orders of magnitude to spare.  On every case the smallest message entry stays above 1e-9 of its vector's largest, so that
no clamp of the sweeps (fmax(., 0); contrib <= 0 -> 1) acts on either side.  The worst error / tolerance is printed (pytest -s).
The joint (max-product) sweep likewise: the oracle's ln L, vectors, arg-max tables and back-traced scenario against joint_pass and
scenario_log_probability, by the assertions tests/test_gpu_joint_shapes.py makes of the device (cases.joint_errors).
"""
import itertools
from decimal import Decimal

import numpy as np
import pytest

import eigen_shape_cases as cases
import f81_exact_ref
import matrix_exact_ref as exact
from oracle import pastml_oracle as orc
from pastml_amd.tree import FlatForest, TreeNode


def test_two_tip_tree_by_hand():
    """L = sum_i pi_i P_a[i, s] P_b[i, u] with P(t) of the oracle (float64); the root's posterior is that sum's terms."""
    k = 5
    rng = np.random.default_rng(1)
    spec = cases.random_spec('EIGEN', k, rng)
    root = TreeNode(name='r', dist=0.0)
    root.add_child(name='a', dist=0.3)
    root.add_child(name='b', dist=0.7)
    flat = FlatForest.from_trees([root])
    masks = np.zeros((3, k), dtype=np.int8)
    masks[0] = 1
    masks[1, 2] = 1
    masks[2, [0, 4]] = 1   # (an ambiguous tip)
    rates = (1.7, 0.01, 0.9)
    Pa, Pb = orc.pij(spec, 0.3, *rates), orc.pij(spec, 0.7, *rates)
    terms = spec['pi'] * Pa[:, 2] * (Pb[:, 0] + Pb[:, 4])
    want = exact.marginal_pass(flat, masks, spec, *rates)
    np.testing.assert_allclose(float(want['loglik']), np.log(terms.sum()), rtol=1e-13)
    np.testing.assert_allclose(want['posterior'][0], terms / terms.sum(), rtol=1e-12)
    np.testing.assert_allclose(want['bu_log10'][0], np.log10(Pa[:, 2] * (Pb[:, 0] + Pb[:, 4])), rtol=0, atol=1e-12)
    assert np.all(want['td_log10'][0] == 0)   # the root's top-down vector of ones
    np.testing.assert_allclose(want['lh_log10'], np.log10(terms.sum()), rtol=1e-12)
    # P(t) on request: rows sum to one as far as A A^-1 of the given doubles is the identity
    P = exact.pij(spec, 0.3, *rates)
    np.testing.assert_allclose(P.astype(float), Pa, rtol=1e-11, atol=1e-15)
    # the joint sweep: max instead of sum
    j = exact.joint_pass(flat, masks, spec, *rates)
    np.testing.assert_allclose(float(j['loglik']), np.log((spec['pi'] * Pa[:, 2] * np.maximum(Pb[:, 0], Pb[:, 4])).max()), rtol=1e-13)
    cols, prod = j['products'][2]
    assert cols == [0, 4]
    np.testing.assert_allclose(prod.astype(float), Pb[:, [0, 4]], rtol=1e-11, atol=1e-15)
    for i in range(k):
        best = int(np.argmax(Pb[i] * masks[2]))
        assert exact.choice_is_a_maximum(j['products'], 2, i, best)
        assert not exact.choice_is_a_maximum(j['products'], 2, i, 4 - best) and not exact.choice_is_a_maximum(j['products'], 2, i, 1)


def test_scenario_log_probability_by_brute_force():
    """Every assignment of states to the three nodes of the tree above: ln(pi_r P_a[r, s_a] P_b[r, s_b]) with P(t) of the oracle, -inf
    where a mask forbids a state; the largest of them is joint_pass's ln L, and joint_pass's other results are those of the tree."""
    k = 5
    rng = np.random.default_rng(1)
    spec = cases.random_spec('EIGEN', k, rng)
    root = TreeNode(name='r', dist=0.0)
    root.add_child(name='a', dist=0.3)
    root.add_child(name='b', dist=0.7)
    flat = FlatForest.from_trees([root])
    masks = np.zeros((3, k), dtype=np.int8)
    masks[0] = 1
    masks[0, 3] = 0   # (a restricted root)
    masks[1, 2] = 1
    masks[2, [0, 4]] = 1
    rates = (1.7, 0.01, 0.9)
    Pa, Pb = orc.pij(spec, 0.3, *rates), orc.pij(spec, 0.7, *rates)
    best = -np.inf
    for r, a, b in itertools.product(range(k), repeat=3):
        got, = exact.scenario_log_probability(flat, masks, spec, *rates, states=[r, a, b])
        if masks[0, r] and masks[1, a] and masks[2, b]:
            want = np.log(spec['pi'][r] * Pa[r, a] * Pb[r, b])
            np.testing.assert_allclose(float(got), want, rtol=1e-11)
            best = max(best, want)
        else:
            assert got == exact.MINUS_INFINITY
    j = exact.joint_pass(flat, masks, spec, *rates)
    np.testing.assert_allclose(float(j['loglik']), best, rtol=1e-12)
    assert len(j['loglik_per_tree']) == 1 and abs(j['loglik_per_tree'][0] - j['loglik']) < Decimal('1e-25')
    v_root = masks[0] * Pa[:, 2] * np.maximum(Pb[:, 0], Pb[:, 4])
    assert np.array_equal(np.isneginf(j['bu_log10']), masks == 0)
    np.testing.assert_allclose(j['bu_log10'][0][masks[0] != 0], np.log10(v_root[masks[0] != 0]), rtol=0, atol=1e-12)
    messages = np.stack([Pa[:, 2], np.maximum(Pb[:, 0], Pb[:, 4])])
    np.testing.assert_allclose(j['min_best_ratio'], (messages.min(axis=1) / messages.max(axis=1)).min(), rtol=1e-10)
    # the scenario of the arg-max choices attains the maximum
    r = int(np.argmax(spec['pi'] * v_root))
    b = 0 if Pb[r, 0] > Pb[r, 4] else 4
    got, = exact.scenario_log_probability(flat, masks, spec, *rates, states=[r, 2, b])
    assert abs(got - j['loglik']) < Decimal('1e-25')   # (the difference is taken at decimal's default 28 digits)


@pytest.mark.parametrize('k', [3, 20])
def test_f81_written_as_an_eigen_model(k):
    """F81's generator diagonalised (generator.py:16-30) and run through the eigen restatement, against tests/f81_exact_ref.py: the two
    differ by the rounding numpy left in d, A and A^-1 only."""
    rng = np.random.default_rng(k)
    flat = FlatForest.random(30, seed=k, max_arity=3, n_trees=2)
    pi = rng.dirichlet(np.ones(k) * 2)
    d, a, ainv = orc.diagonalise(pi)
    masks = cases.random_masks(flat, k, rng)
    rates = (1.3, 0.02, 0.9)
    got = exact.marginal_pass(flat, masks, dict(kind=2, pi=pi, d=d, A=a, Ainv=ainv), *rates)
    want = f81_exact_ref.marginal_pass(flat, masks, pi, *rates, top_down=True)
    assert abs(got['loglik'] - want['loglik']) < Decimal('1e-11') * abs(want['loglik'])
    np.testing.assert_allclose(got['posterior'], want['posterior'], rtol=1e-11, atol=1e-300)
    for key in ('bu_log10', 'td_log10'):
        assert np.array_equal(np.isneginf(got[key]), np.isneginf(want[key]))
        fin = np.isfinite(want[key])
        np.testing.assert_allclose(got[key][fin], want[key][fin], rtol=0, atol=1e-11)


def test_hky_with_kappa_one_and_equal_frequencies_is_jc():
    """kappa = 1 makes HKY the F81 model of its frequencies; with pi = 1/4 (exact doubles) both restatements compute JC in exact
    arithmetic, so they agree to their own 50 digits, not to float64."""
    rng = np.random.default_rng(4)
    flat = FlatForest.random(40, seed=4, max_arity=3, n_trees=2)
    pi = np.full(4, 0.25)
    masks = cases.random_masks(flat, 4, rng)
    rates = (2.1, 0.01, 0.9)
    got = exact.marginal_pass(flat, masks, dict(kind=1, pi=pi, kappa=1.0), *rates)
    want = f81_exact_ref.marginal_pass(flat, masks, pi, *rates, top_down=True)
    assert abs(got['loglik'] - want['loglik']) < Decimal('1e-40') * abs(want['loglik'])
    np.testing.assert_allclose(got['posterior'], want['posterior'], rtol=1e-15, atol=0)
    np.testing.assert_allclose(got['bu_log10'], want['bu_log10'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got['td_log10'], want['td_log10'], rtol=0, atol=1e-12)


def test_hky_transition_matrix_against_the_oracle():
    rng = np.random.default_rng(7)
    spec = cases.random_spec('HKY', 4, rng)
    for t in (0.01, 0.3, 5.):
        np.testing.assert_allclose(exact.pij(spec, t, 1.4, 0.01, 0.9).astype(float), orc.pij(spec, t, 1.4, 0.01, 0.9), rtol=1e-13)


def oracle_ratios(flat, masks, spec, rates, want, k):
    assert want['loglik'].is_finite()
    assert want['min_message_ratio'] > cases.MIN_MESSAGE_RATIO
    r = orc.full_marginal_pass(flat, masks.astype(int), spec, *rates)
    return cases.ratios(cases.errors(cases.oracle_as_logs(r), want), k)


SHAPE_CASES = [(k, 'S') for k in cases.CPU_STATES + cases.STATES_ONE_MATRIX] + [(k, 'L') for k in cases.CPU_STATES_L]


@pytest.mark.parametrize('k,which', SHAPE_CASES)
def test_oracle_stays_inside_the_tolerances_of_the_shape_tests(k, which):
    """ln L (LNL_RTOL), the vectors in log10 (LOG10_ATOL; 1e-9 beyond 64 states), posteriors (POST_RTOL) and the nodes' likelihood sums
    of the oracle against the exact pass, both columns of a case of tests/test_gpu_eigen_shapes.py."""
    b = cases.build(k, which)
    flat = b['flat']
    assert np.all(b['masks'][0][flat.is_tip].sum(axis=1) == 1)   # column 0: every tip observed
    assert np.all(flat.dist[flat.parent >= 0] > 0)
    worst = {}
    for c in range(2):
        for key, x in oracle_ratios(flat, b['masks'][c], b['specs'][c], b['rates'][c], cases.exact_pass(k, which, c), k).items():
            worst[key] = max(worst.get(key, 0.0), x)
    print('k = {} forest {}: worst error / tol of the oracle: {}'.format(k, which, ', '.join('{} {:.3g}'.format(a, worst[a])
                                                                                              for a in sorted(worst))))
    assert max(worst.values()) < 1, worst


DEEP_CASES = [('EIGEN', 11), ('EIGEN', 16), ('EIGEN', 20), ('EIGEN', 40), ('EIGEN', 43), ('EIGEN', 64), ('EIGEN', 65), ('HKY', 4)]


@pytest.mark.parametrize('kind,k', DEEP_CASES)
def test_oracle_on_the_deep_caterpillars(kind, k):
    d = cases.deep_caterpillar(kind, k)
    want = cases.deep_exact(kind, k)
    root_log2 = want['bu_log10'][0].max() * exact.LOG2_OF_10
    assert d['depth'] % 50 == 0 and root_log2 < cases.DEEP_LOG2 and abs(root_log2 - d['root_log2_exact']) < 1e-6
    worst = oracle_ratios(d['flat'], d['masks'], d['spec'], d['rates'], want, k)
    print('{} k = {}, depth {} (log2 of the root\'s vector {:.0f}): worst error / tol of the oracle: {}'.format(
        kind, k, d['depth'], root_log2, ', '.join('{} {:.3g}'.format(a, worst[a]) for a in sorted(worst))))
    assert max(worst.values()) < 1, worst


@pytest.mark.parametrize('k', [5, 20])
def test_oracle_on_the_forest_of_polytomies(k):
    d = cases.polytomy_forest(k)
    want = cases.polytomy_exact(k)
    assert np.all(want['bu_log10'][d['polytomies']].max(axis=1) * exact.LOG2_OF_10 < -200)
    worst = oracle_ratios(d['flat'], d['masks'], d['spec'], d['rates'], want, k)
    print('k = {}, polytomies of {} tips: worst error / tol of the oracle: {}'.format(
        k, d['fan'], ', '.join('{} {:.3g}'.format(a, worst[a]) for a in sorted(worst))))
    assert max(worst.values()) < 1, worst


# ---------------------------------------------------------------------------------------------------------------------
# the joint sweep
# ---------------------------------------------------------------------------------------------------------------------
def oracle_joint_ratios(label, flat, masks, spec, rates, want):
    """The oracle against the exact joint pass, by the assertions the device gets (tests/test_gpu_joint_shapes.py): the preconditions,
    tables / zero patterns / masks (cases.joint_errors), then error / tolerance of ln L (LNL_RTOL), the vectors (LOG10_ATOL) and
    the scenario (nodes of the tree x 1e-12 in ln)."""
    assert want['loglik'].is_finite() and want['min_best_ratio'] > cases.MIN_MESSAGE_RATIO, want['min_best_ratio']
    err = cases.joint_errors(cases.oracle_joint(flat, masks, spec, rates), want, flat, masks, spec, rates)
    ratio = dict(lnl=err['lnl'] / cases.LNL_RTOL, log10=err['log10'] / cases.LOG10_ATOL, scenario=err['scenario'])
    print('{}: oracle, joint: {}'.format(label, '  '.join('{} {:.3g} ({:.3g} of tol)'.format(a, err[a], ratio[a]) for a in sorted(err))))
    return ratio


JOINT_CASES = [(k, 'S') for k in cases.CPU_STATES] + [(k, 'J') for k in cases.CPU_STATES_L]


@pytest.mark.parametrize('k,which', JOINT_CASES)
def test_oracle_joint_sweep_stays_inside_the_tolerances_of_the_joint_shape_tests(k, which):
    """Forest S and the level forest J(k), both columns."""
    b = cases.build_joint(k, which)
    flat = b['flat']
    assert np.all(b['masks'][0][flat.is_tip].sum(axis=1) == 1)
    if which == 'J' and k <= 32:
        assert cases.j_passes(k, cases.j_cherries(k)) == (3, 1) and cases.j_tip_chunk_passes(k, flat.n_tips) > 1
    for c in range(2):
        ratio = oracle_joint_ratios('k = {} forest {} column {}'.format(k, which, c), flat, b['masks'][c], b['specs'][c], b['rates'][c],
                                    cases.joint_exact(k, which, c))
        assert max(ratio.values()) < 1, ratio


@pytest.mark.parametrize('k', [65, 128, 129])
def test_oracle_joint_sweep_beyond_64_states(k):
    b = cases.build_joint(k, 'T')
    assert b['masks'][0][b['flat'].is_tip].sum() == b['flat'].n_tips and b['masks'][1][b['flat'].is_tip].sum() == b['flat'].n_tips - 1 + k
    for c in range(2):
        ratio = oracle_joint_ratios('k = {} forest T column {}'.format(k, c), b['flat'], b['masks'][c], b['specs'][c], b['rates'][c],
                                    cases.joint_exact(k, 'T', c))
        assert max(ratio.values()) < 1, ratio


@pytest.mark.parametrize('which', ['S', 'J'])
def test_oracle_joint_sweep_of_hky(which):
    b = cases.build_joint(4, which, 'HKY')
    assert which == 'S' or list(np.diff(b['flat'].bu_offsets)) == [cases.HKY_J_CHERRIES, 2, 1]
    for c in range(2):
        ratio = oracle_joint_ratios('HKY forest {} column {}'.format(which, c), b['flat'], b['masks'][c], b['specs'][c], b['rates'][c],
                                    cases.joint_exact(4, which, c, 'HKY'))
        assert max(ratio.values()) < 1, ratio


@pytest.mark.parametrize('kind,k', [('EIGEN', 11), ('EIGEN', 20), ('EIGEN', 43), ('HKY', 4)])
def test_oracle_joint_sweep_on_the_deep_caterpillars(kind, k):
    """The max-product vectors lie below the sum vectors: the root is below 2^-800 here too."""
    d = cases.deep_caterpillar(kind, k)
    want = cases.deep_joint_exact(kind, k)
    assert want['bu_log10'][0].max() * exact.LOG2_OF_10 < cases.DEEP_LOG2
    ratio = oracle_joint_ratios('deep {} k = {} depth {}'.format(kind, k, d['depth']), d['flat'], d['masks'], d['spec'], d['rates'], want)
    assert max(ratio.values()) < 1, ratio


@pytest.mark.parametrize('k', [5, 20])
def test_oracle_joint_sweep_on_the_forest_of_polytomies(k):
    d = cases.polytomy_forest(k)
    want = cases.polytomy_joint_exact(k)
    assert np.all(want['bu_log10'][d['polytomies']].max(axis=1) * exact.LOG2_OF_10 < -200)
    ratio = oracle_joint_ratios('polytomies k = {} fan {}'.format(k, d['fan']), d['flat'], d['masks'], d['spec'], d['rates'], want)
    assert max(ratio.values()) < 1, ratio
