"""
CPU tests of tests/degenerate_forest_cases.py, the inputs of tests/test_gpu_degenerate_forests.py: what each forest is claimed to
contain (the census, in the planner's terms), the widths of `crowd` against the narrow limits the planners use, a finite exact
ln L and no clamped message on every case the device runs, the oracle held to the exact passes by the checkers and at the
tolerances of the GPU file, and the sensitivity of those checkers to a unary node that a kernel skipped or merged.  Matrix models
beyond 64 states are held to the oracle on `shapes` only (an exact pass of `crowd` at 65 states takes 20 s).
"""
import numpy as np
import pytest

import degenerate_forest_cases as cases
import eigen_shape_cases as eigen_cases
from oracle import pastml_oracle as orc
from test_gpu_parity import LNL_RTOL


def test_shapes_holds_every_shape_it_names():
    flat = cases.forest('shapes')
    c = cases.census(flat)
    h = c['histogram']
    assert c['lone_tips'] == 3 and c['n_trees'] == 12 + len(cases.STARS)
    assert h[1] == c['unary'] == 13 and c['unary_roots'] == 3 and c['unary_chains'] == 4
    assert all(h[s] >= 1 for s in cases.STARS) and c['widest_arity'] == 17 and list(h[14:18]) == [1, 1, 1, 1]
    # a root with one tip is a stored node; the one-tip cherries: under the unary root, beside the cherry of two, beside the
    # five-tip and the two-tip cherry
    assert c['one_tip_cherries'] == 4 and c['unary_over_tip'] == 5
    assert c['both_code2'] == 1 and c['one_tip_cherry_ok'] == 3
    assert c['unary_over_stored'] >= 3 and c['two_level_roots'] == 2 and c['zero_branches'] == 0
    nc, fc = flat.n_children, flat.first_child
    above = [i for i in range(flat.n_nodes) if nc[i] == 1 and nc[fc[i]] == 2 and cases.census_is_two_level(flat, int(fc[i]))]
    beside = [i for i in range(flat.n_nodes) if nc[i] == 2 and nc[fc[i]] == 1 and cases.census_is_two_level(flat, int(fc[i]) + 1)]
    assert len(above) == 1 and len(beside) == 1
    three = [i for i in range(flat.n_nodes) if nc[i] == 1 and nc[fc[i]] == 3 and flat.parent[i] >= 0]
    assert len(three) == 1


def test_crowd_is_wider_than_every_narrow_limit():
    flat = cases.forest('crowd')
    c = cases.census(flat)
    each = cases.CROWD_EACH
    assert c['n_trees'] == 4 * each + 1 and c['lone_tips'] == each and c['unary_roots'] == 2 * each and c['unary'] == 3 * each
    assert c['unary_over_stored'] == each and c['unary_over_tip'] == each and c['unary_chains'] == each
    assert c['histogram'][2] >= 2 * each and c['n_nodes'] > 1000
    big = np.flatnonzero(np.bincount(flat.tree_id) > 5)
    assert len(big) == 1 and abs(int(big[0]) - 2 * each) <= 1, 'the 40-tip tree sits in the middle'
    # the four kinds are mixed, not in blocks: no run of one kind longer than a tenth of it
    kinds = np.bincount(flat.tree_id)[:2 * each]
    runs = np.diff(np.flatnonzero(np.diff(kinds) != 0))
    assert runs.max() < each // 10 * 2
    # the levels next to the roots: the roots themselves (top-down depth 0), their children (depth 1) and the plain level of the
    # nodes over tips (bottom-up level 0), against the widest narrow limit any sweep uses at two columns
    C = 2
    limits = [cases.NARROW_GEMM, cases.plain_narrow_limit(C)]
    limits += [eigen_cases.joint_narrow_limit(k) for k in cases.EIGEN_STATES + cases.EIGEN_STATES_SHAPES_ONLY if k <= 64]
    limits += [cases.f81_narrow_limit(C, g) for g in (1, 2, 4, 8, 16, 32, 64)]
    widest = max(limits)
    assert widest == 256
    assert c['td_widths'][0] > widest and c['td_widths'][1] > widest and c['bu_widths'][0] > widest
    # ... under cherry fusion (the F81 family): the stored nodes of fused height 1 are the roots over tips and the unary nodes
    # over cherries
    assert 3 * each > widest
    # td_roots_kernel walks WAVES_PER_BLOCK * 64 / G roots per workgroup: at the smallest G (2 lanes, 2 states) the roots span
    # more than one workgroup's pass (the grid covers every root once: a second pass of one workgroup needs GRID_CAP)
    assert c['n_trees'] > cases.WAVES_PER_BLOCK * (64 // 2)


@pytest.mark.parametrize('zeros', [False, True])
def test_grafted_has_unary_nodes_of_every_kind(zeros):
    flat = cases.forest('grafted', zeros)
    base = cases.contracted(flat)[0]
    c, c0 = cases.census(flat), cases.census(base)
    assert c0['unary'] == 0 and c0['n_nodes'] == c['n_nodes'] - c['unary'] and 170 <= flat.n_tips <= 230
    assert c0['two_level_roots'] >= 15 and c0['widest_arity'] >= 3
    assert c['unary'] >= 30 and c['unary_chains'] >= 4 and c['unary_over_tip'] >= 8 and c['unary_over_stored'] >= 8
    assert c['one_tip_cherries'] == c['unary_over_tip'] and c['unary_roots'] == 0
    # some clumps keep the two-level pattern, most carry a unary node inside
    assert 2 <= c['two_level_roots'] < c0['two_level_roots']
    assert (c['zero_branches'] >= 5) == zeros and (zeros or c['zero_branches'] == 0)
    if zeros:
        inserted = flat.n_children == 1
        assert ((flat.dist == 0) & ~inserted & (flat.parent >= 0)).sum() == 0, 'a zero branch that is not an inserted one'


@pytest.mark.parametrize('kind, k, name', cases.CASES, ids=cases.IDS)
def test_inputs_are_what_the_columns_claim(kind, k, name):
    b = cases.build(kind, k, name)
    flat, masks = b['flat'], b['masks']
    nc = flat.n_children
    assert np.all(masks[0][flat.is_tip].sum(axis=1) == 1) and np.all(masks[0][~flat.is_tip] == 1)
    assert b['rates'][0][1:] == (0.0, 1.0) and b['rates'][1][1] > 0 and b['rates'][1][2] < 1
    tips = masks[1][flat.is_tip].sum(axis=1)
    assert (tips == k).any() and (tips == 1).any() and (k == 2 or (tips == 2).any())
    assert nc[b['restricted_unary']] == 1 and masks[1][b['restricted_unary']].sum() == 1
    assert flat.parent[b['restricted_root']] < 0 and masks[1][b['restricted_root']].sum() == 1
    assert (masks[1][~flat.is_tip].sum(axis=1) == 1).sum() >= 2
    lone = flat.roots[nc[flat.roots] == 0]
    if name != 'grafted':
        assert masks[1][lone[0]].sum() == 1 and masks[1][lone[1]].sum() == k and masks[1][lone[2]].sum() == 2
    else:
        assert len(lone) == 0
    if kind != 'F81':
        assert np.all(flat.dist[flat.parent >= 0] > 0)


HOST = [c for c in cases.CASES if c[0] == 'F81' or c[1] <= 64 or c[2] == 'shapes']


@pytest.mark.parametrize('kind, k, name', HOST, ids=['{}{}-{}'.format(*c) for c in HOST])
def test_oracle_against_exact_arithmetic(kind, k, name):
    """A finite exact ln L, no message near a clamp, every tree with or without information (cases.flat_nodes), and the oracle in
    tolerance on both columns of the marginal pass and of the joint sweep -- by the checkers of the GPU file."""
    b = cases.build(kind, k, name)
    flat = b['flat']
    worst = {}
    for c in range(2):
        want, joint = cases.exact_pass(kind, k, name, c), cases.joint_exact(kind, k, name, c)
        assert want['loglik'].is_finite() and joint['loglik'].is_finite()
        if kind != 'F81':
            assert want['min_message_ratio'] > eigen_cases.MIN_MESSAGE_RATIO and joint['min_best_ratio'] > eigen_cases.MIN_MESSAGE_RATIO
        still = cases.flat_nodes(want)
        assert still.any() == (c == 1 and name != 'grafted')
        args = (flat, b['masks'][c], b['specs'][c], b['rates'][c])
        r = orc.full_marginal_pass(flat, b['masks'][c].astype(int), b['specs'][c], *b['rates'][c])
        ratios = cases.marginal_ratios(kind, k, cases.oracle_as_device(r), want, flat)
        ratios.update({'joint_' + q: v for q, v in cases.joint_ratios(kind, k, cases.oracle_joint(kind, *args), joint, *args).items()})
        for q, v in ratios.items():
            worst[q] = max(worst.get(q, 0.0), v)
    print('degenerate | oracle {:5s} k={:3d} {:7s} | '.format(kind, k, name) + ' '.join('{} {:.3g}'.format(q, worst[q]) for q in sorted(worst)))
    assert max(worst.values()) < 1, worst


SENSITIVITY = [('F81', 4), ('F81', 33), ('EIGEN', 5), ('HKY', 4)]


@pytest.mark.parametrize('name', cases.FORESTS)
@pytest.mark.parametrize('kind, k', SENSITIVITY, ids=['{}{}'.format(*s) for s in SENSITIVITY])
def test_a_skipped_unary_node_cannot_pass(kind, k, name):
    """Column 1 (tau > 0: every branch is lengthened by tau, so two branches in a row are not their sum): the exact ln L of the
    forest without its unary nodes differs from the exact ln L by more than 1000 times its tolerance, and the checker of the
    marginal pass, handed the exact results with that ln L in their place, reports it."""
    b = cases.build(kind, k, name)
    flat, c = b['flat'], 1
    small, kept = cases.contracted(flat)
    assert cases.census(small)['unary'] == 0 and small.n_nodes < flat.n_nodes and len(small.roots) == len(flat.roots)
    want = cases.exact_pass(kind, k, name, c)
    other = cases.exact_marginal(kind, small, b['masks'][c][kept], b['specs'][c], b['rates'][c])
    assert other['loglik'].is_finite()
    # the exact pass of `flat` itself in the device's terms: it passes; with the other ln L it fails by a factor 1000
    lh = 10.0 ** want['lh_log10']
    with np.errstate(over='ignore', under='ignore'):
        got = dict(lnl=float(want['loglik']), bu=10.0 ** want['bu_log10'], bu_sf=np.zeros(flat.n_nodes), td=10.0 ** want['td_log10'],
                   td_sf=np.zeros(flat.n_nodes), posterior=want['posterior'], lh_sum=lh, lh_sf=np.zeros(flat.n_nodes))
    assert cases.marginal_ratios(kind, k, got, want, flat)['lnl'] < 1e-3
    wrong = cases.marginal_ratios(kind, k, dict(got, lnl=float(other['loglik'])), want, flat)
    assert wrong['lnl'] > 1000, wrong
    assert abs(float(other['loglik'] - want['loglik'])) > 1000 * LNL_RTOL * abs(float(want['loglik']))


@pytest.mark.parametrize('seed', range(cases.RANDOM_SEEDS))
def test_random_draws_have_unary_nodes_and_a_reference(seed):
    """Every draw of the random section has a unary node, and the reference has an answer for it -- a likelihood or a
    zero-likelihood report, never the empty-minimum failure that the fuzz skips on."""
    kind, k, flat, specs, rates, masks = cases.draw_random_case(seed)
    c = cases.census(flat)
    assert c['unary'] > 0 and 3 <= flat.n_tips <= 140
    for col in range(len(specs)):
        try:
            orc.full_marginal_pass(flat, masks[col].astype(int), specs[col], *rates[col])
        except orc.OracleLikelihoodError:
            pass


def test_random_draws_cover_the_kinds_and_small_trees():
    draws = [cases.draw_random_case(seed) for seed in range(cases.RANDOM_SEEDS)]
    assert {d[0] for d in draws} == {'F81', 'EIGEN', 'HKY'}
    stats = [cases.census(d[2]) for d in draws]
    assert sum(s['lone_tips'] > 0 for s in stats) >= 12 and sum(s['unary_roots'] > 0 for s in stats) >= 12
    assert sum(s['zero_branches'] > 0 for s in stats) >= 3 and sum(s['unary_chains'] > 0 for s in stats) >= 12
