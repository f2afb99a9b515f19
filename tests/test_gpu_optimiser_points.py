"""
GPU tests of the optimiser's own column blocks -- CharacterBatch.open_optimiser / evaluate_points (submit_points, stage_f81,
commit_f81, the per-column mask variants, sweeps of the active columns only), as fit_parameters_steps drives them -- at the
optimiser's own parameter values, against exact arithmetic (tests/f81_exact_ref.py).

With tau free one finite-difference block holds a base point at tau = 0 (altered masks) next to its tau-step point at 1e-8
(plain masks), beside the sf and frequency steps.  On a zero-length branch at tau = 1e-8 the sweeps form 1 - exp(-mu t') with
mu t' of 1e-11 .. 1e-7: float64 is no reference there (the oracle's own ln L is off by up to 3e-6), so the tolerance is derived,

    tol = LNL_RTOL |L| + 2^-53 G,      G = sum over the branches with e_n < 1 of 1 / (1 - e_n):

an exponential within one unit in the last place is off by at most 2^-53 for e < 1, 1 - e is then exact, a branch's message carries
a relative error of at most 2^-53 / (1 - e_n), and ln L adds these up.  Away from zero-length branches G is about N and tol is
the suite's usual 1e-11.  tests/test_f81_exact_ref.py holds the oracle to the same tolerance on the same inputs (CPU).
"""
import numpy as np
import pytest

import f81_exact_ref as exact
import optimiser_point_cases as cases
from pastml_amd import hip
from pastml_amd.batch import LikelihoodError, masks_from_words
from pastml_amd.models import PointBlock, KIND_F81
from test_gpu_parity import LEVEL_SCHEDULE, LNL_RTOL, POST_RTOL

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def reversed_block(block):
    if type(block) is PointBlock:
        return PointBlock(KIND_F81, np.ascontiguousarray(block.pi[::-1]), block.sf[::-1].copy(), block.tau[::-1].copy(),
                          block.tf[::-1].copy())
    return list(block)[::-1]


def check_block(b, c, block, values, worst, what):
    """ln L of every column of a block within tol of the exact value; no LikelihoodError where the exact likelihood is positive."""
    assert not isinstance(values, LikelihoodError), '{}: {}'.format(what, values)
    pi, sf, tau, tf = cases.as_arrays(block)
    avg = b['stats'].avg_nonzero_brlen
    for j in range(len(sf)):
        masks = cases.column_masks(b['batch'], c, tau[j], b['altered'][c])
        want = cases.exact_value(b, c, masks, pi[j], sf[j], tau[j], tf[j])
        assert want['loglik'].is_finite()
        ratio = exact.error_ratio(values[j], want, LNL_RTOL)
        key = cases.regime(tau[j], avg)
        worst[key] = max(worst.get(key, 0.0), ratio)
        assert ratio < 1, '{}: character {} point {} (sf {!r}, tau {!r}): ln L {!r}, exact {:.20}, error / tol {:.3g}' \
            .format(what, c, j, sf[j], tau[j], values[j], want['loglik'], ratio)


@pytest.mark.parametrize('schedule', ['default', 'levels'])
@pytest.mark.parametrize('k,family', cases.CASES)
def test_blocks_at_the_optimisers_points(k, family, schedule):
    run_blocks(cases.build(k, family), schedule)


@pytest.mark.parametrize('k,family', cases.CLUMP_CASES)
def test_blocks_through_two_level_and_stacked_units(k, family):
    """The random forest above has no node of the shape the two-level units take (its level schedule runs plain units only, as
    the counts it prints say): the same blocks on a small forest of balanced clumps, where both kinds of units are scheduled."""
    ran = run_blocks(cases.build(k, family, 'clumps'), 'levels')
    on, n_two, n_stacked = ran[1]
    assert on and n_two > 0 and n_stacked > 0, ran


def run_blocks(b, schedule):
    k, family = b['k'], b['family']
    batch = b['batch']
    assert b['altered'][0] is not None   # (the zero-branch alteration changes character 0's masks: both variants are in play)
    w = cases.width(b)
    # 'levels': LEVEL_SCHEDULE, and no single-launch kernel for this forest of some 200 nodes (it takes every forest of up to 2048
    # nodes whatever the other switches say), so that the level launches with their two-level and stacked units run
    opt = batch.open_optimiser([w, w], tune=dict(LEVEL_SCHEDULE, SMALL_MAX_NODES=0) if schedule == 'levels' else None)
    eng, offsets = opt['engine'], opt['offsets']
    worst = {}
    ran = None
    try:
        for i, (sf0, tau0) in enumerate(cases.base_points(b['stats'])):
            blocks = {c: cases.block_at(b['models'][c], sf0, tau0) for c in range(2)}
            n = len(blocks[0])
            # one block at a time, both in one sweep, then a request of one block only (the other sits the sweep out)
            alone = {c: batch.evaluate_points({c: blocks[c]})[c] for c in range(2)}
            both = batch.evaluate_points(blocks)
            if ran is None:
                ran = eng.sweep_schedule(), eng.schedule_info()
                # (default: the single-launch kernel up to 256 states; 'levels': level launches, with units where the forest
                # has them)
                assert schedule == 'default' or ran[0][0] in (hip.SCHEDULE_LEVELS, hip.SCHEDULE_TWO_LEVEL), ran
            for c in range(2):
                check_block(b, c, blocks[c], both[c], worst, 'staged')
                assert same_bits(alone[c], both[c])
            asks, idle = i % 2, 1 - i % 2
            again = batch.evaluate_points({asks: blocks[asks]})
            assert list(again) == [asks] and same_bits(again[asks], both[asks])
            assert same_bits(eng._lnl[offsets[idle]:offsets[idle] + n], both[idle])
            if tau0 == 0:
                # the tau = 0 and tau > 0 points change places, and back: a column's mask variant follows its tau
                assert (blocks[0].tau == 0).any() and (blocks[0].tau != 0).any()
                swapped = batch.evaluate_points({c: reversed_block(blocks[c]) for c in range(2)})
                back = batch.evaluate_points(blocks)
                for c in range(2):
                    assert same_bits(swapped[c], both[c][::-1])
                    assert same_bits(back[c], both[c])
            # the tuple path: (spec, rates) per point with a different pi per point, as under frequency smoothing
            tuples = {c: cases.block_at(b['smoothing'][c], sf0, tau0) for c in range(2)}
            assert all(type(p) is list and len(p) == cases.SMOOTHING_POINTS for p in tuples.values())
            listed = batch.evaluate_points(tuples)
            for c in range(2):
                check_block(b, c, tuples[c], listed[c], worst, 'tuples')
            if tau0 == 0:
                swapped = batch.evaluate_points({c: reversed_block(tuples[c]) for c in range(2)})
                for c in range(2):
                    assert same_bits(swapped[c], listed[c][::-1])
            staged = batch.evaluate_points({c: cases.as_point_block(tuples[c]) for c in range(2)})
            for c in range(2):
                assert same_bits(staged[c], listed[c])
    finally:
        batch.close()
    print('k = {} {} {} (sweep schedule {}; units on, two-level nodes, stacked nodes {}): worst error / tol of the device per '
          'regime of tau: {}'.format(k, family, schedule, ran[0], ran[1],
                                     ', '.join('{} {:.3g}'.format(a, worst[a]) for a in sorted(worst))))
    return ran


def test_f81_pij_at_small_arguments():
    """Every entry of P(t) relative to the exact entry within 2^-53 / (1 - e) + 4 * 2^-53, down to mu t' = 1e-11 (the absolute
    2e-15 of test_pij_matches_reference swallows the off-diagonal entries there whole)."""
    k = 5
    flat, _ = cases.forest()
    pi = np.random.default_rng(5).dirichlet(np.ones(k) * 3)
    mu = 1. / (1. - pi.dot(pi))
    ts = np.array([1e-11, 1e-9, 1e-7, 1e-3, 1., 40.]) / mu
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([(dict(kind=0, pi=pi), (1., 0., 1.))])
        got = eng.pij(ts)
    for t, P in zip(ts, got):
        want, e = exact.pij(pi, t)
        with exact.decimal.localcontext(exact._CONTEXT):
            bound = exact.U53 / (1 - e) + 4 * exact.U53
            for i in range(k):
                for j in range(k):
                    err = abs(exact.Decimal(float(P[i, j])) - want[i][j]) / want[i][j]
                    assert err <= bound, 'mu t = {:.3g}: P[{}][{}] = {!r}, exact {:.20}, relative error {:.3g} > {:.3g}' \
                        .format(mu * t, i, j, P[i, j], want[i][j], err, bound)


@pytest.mark.parametrize('k,family', [(5, 'F81'), (64, 'EFT')])
def test_marginal_pass_at_the_optimisers_base_points(k, family):
    """Posteriors at the nine base points against the exact ones: relative POST_RTOL + 2 * 2^-53 G for entries above 1e-300 (the
    bottom-up and the top-down vector of a node each carry the branches' errors once), zeros where the exact ones are zero."""
    b = cases.build(k, family)
    batch, models = b['batch'], b['models']
    flat, _ = cases.forest()
    plain = batch.masks.copy()
    try:
        for sf0, tau0 in cases.base_points(b['stats']):
            for m in models:
                m._sf, m._tau = sf0, tau0
                m.calc_tau_factor()
            if tau0 == 0:
                batch.alter(np.ones(2, dtype=bool))   # (as ml_acr does before its marginal pass, ml.py:700-703)
            lnl, post, _, _ = batch.marginal_pass(models)
            for c in range(2):
                masks = masks_from_words(batch.masks[c], k)
                want = exact.marginal_pass(flat, masks, np.asarray(models[c].frequencies), *models[c].rate_params(),
                                           top_down=True, vectors=False)
                assert exact.error_ratio(lnl[c], want, LNL_RTOL) < 1
                rtol = POST_RTOL + 2 * U53 * float(want['G'])
                assert np.array_equal(post[c] == 0, want['posterior'] == 0)
                big = want['posterior'] > 1e-300
                np.testing.assert_allclose(post[c][big], want['posterior'][big], rtol=rtol, atol=0)
            batch.masks[:] = plain
    finally:
        batch.masks[:] = plain
        batch.close()
