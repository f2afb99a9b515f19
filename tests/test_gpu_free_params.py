"""
GPU tests of the two acr() arguments that change the optimiser's parameter vector -- tau=None (the pipeline's smoothing=True:
tau is optimised) and frequency_smoothing=True -- against runs of the real reference on Albania / Country, MPPA
(tests/golden/albania_free_params.npz, written by tests/golden/make_golden.py albania_free_params).

Every reference run is stored three times: as it is, and with every L-BFGS-B start multiplied by (1 + 1e-12) and (1 - 1e-12).
Five of the six runs are stable under that and are compared end to end.  F81 with tau=None is not -- the reference's own ln L
moves from -110.606 to -116.025 when its starts move by a rounding error -- so it is compared as a function: every vector the
reference's objective was asked at, in order, through CharacterBatch.evaluate_points, against the value it returned.
"""
import os

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden, GOLDEN
from pastml_amd.acr import acr, calculate_observed_freqs
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.batch import CharacterBatch, LikelihoodError, annotation_words, block_width
from pastml_amd.ml import MPPA, LOG_LIKELIHOOD, RESTRICTED_LOG_LIKELIHOOD_FORMAT_STR, MARGINAL_PROBABILITIES, MODEL
from pastml_amd.models import PointBlock
from pastml_amd.models.F81Model import F81Model, F81
from pastml_amd.models.JCModel import JC
from pastml_amd.models.EFTModel import EFT
from pastml_amd.tree import read_tree, FlatForest, get_flat_forest
from test_gpu_parity import LNL_RTOL

pytestmark = pytest.mark.gpu

DATA = os.path.join(GOLDEN, 'data')
TREE_NWK = os.path.join(DATA, 'Albanian.tree.152tax.tre')
COUNTRY = 'Country'
REPEATS = ('', 'plus_', 'minus_')


def country_df():
    return pd.read_csv(os.path.join(DATA, 'data.txt'), index_col=0, header=0)[[COUNTRY]]


def run_kwargs(z, name):
    given = {COUNTRY: {str(s): float(f) for s, f in zip(z['states'], z['observed_frequencies'])}}
    return {'JC_tau': dict(model=JC, tau=None),
            'EFT_tau': dict(model=EFT, tau=None),
            'F81_tau': dict(model=F81, tau=None),
            'F81_fs': dict(model=F81, frequency_smoothing=True),
            'F81_given_fs': dict(model=F81, frequency_smoothing=True, column2parameters=given),
            'F81_given_fs_tau': dict(model=F81, frequency_smoothing=True, column2parameters=given, tau=None)}[name]


def run_acr(df, **kwargs):
    np.random.seed(239)
    tree = read_tree(TREE_NWK)
    return tree, acr(tree, df, prediction_method=MPPA, **kwargs)


def selected(tree, res, column):
    nodes = FlatForest.from_trees([tree]).nodes
    s2i = {s: i for i, s in enumerate(res['states'])}
    sel = np.zeros((len(nodes), len(s2i)), dtype=np.int8)
    for i, n in enumerate(nodes):
        for s in getattr(n, column):
            sel[i, s2i[s]] = 1
    return nodes, sel


@pytest.mark.parametrize('name', ['JC_tau', 'EFT_tau', 'F81_fs', 'F81_given_fs', 'F81_given_fs_tau'])
def test_stable_runs_match_the_reference(name):
    """The tolerances of test_acr_mppa_albania_matches_reference_run, or four times the reference's own spread over its three
    repeats where that is larger; tau ends at 0.0 exactly; the selected states are the reference's wherever its repeats agree."""
    z = load_golden('albania_free_params')
    tree, results = run_acr(country_df(), **run_kwargs(z, name))
    res = results[0]

    def ref(key):
        return z['{}_{}'.format(name, key)]

    def spread(key):
        values = np.stack([np.asarray(z['{}_{}{}'.format(name, r, key)], dtype=np.float64) for r in REPEATS])
        return float((values.max(axis=0) - values.min(axis=0)).max())

    print('{}: ln L {!r} (reference {!r}, spread {:.3g}), sf {!r} (reference {!r}, spread {:.3g}), tau {!r}'
          .format(name, res[LOG_LIKELIHOOD], float(ref('loglik')), spread('loglik'), res[MODEL].sf, float(ref('sf')),
                  spread('sf'), res[MODEL].tau))
    assert res[MODEL].tau == 0.0 and float(ref('tau')) == 0.0
    np.testing.assert_allclose(res[LOG_LIKELIHOOD], ref('loglik'), rtol=0, atol=max(2e-6, 4 * spread('loglik')))
    np.testing.assert_allclose(res[MODEL].sf, ref('sf'), rtol=0, atol=max(2e-4 * float(ref('sf')), 4 * spread('sf')))
    np.testing.assert_allclose(res[MODEL].frequencies, ref('frequencies'), rtol=0, atol=max(2e-5, 4 * spread('frequencies')))
    key = 'loglik_restricted_' + MPPA
    np.testing.assert_allclose(res[RESTRICTED_LOG_LIKELIHOOD_FORMAT_STR.format(MPPA)], ref(key), rtol=0,
                               atol=max(1e-4, 4 * spread(key)))
    nodes, sel = selected(tree, res, COUNTRY)
    mps = res[MARGINAL_PROBABILITIES]
    assert list(mps.index) == [n.name for n in nodes] and list(mps.columns) == list(ref('states'))
    np.testing.assert_allclose(mps.values, ref('posterior'), rtol=0, atol=max(2e-5, 4 * spread('posterior')))
    theirs = np.stack([z['{}_{}selected_mppa'.format(name, r)] for r in REPEATS])
    agreed = (theirs == theirs[0]).all(axis=(0, 2))
    assert agreed.sum() > 0.9 * len(nodes)
    assert np.array_equal(sel[agreed], theirs[0][agreed])


def three_column_df(z):
    df = pd.DataFrame(z['three_values'], index=z['three_index'], columns=z['three_columns'])
    return df.replace('', np.nan)


def test_only_the_first_character_optimises_tau():
    """acr(tau=None) over three characters: the first maximum-likelihood character gets the free tau, the argument is 0 from then
    on (pastml/acr.py:185-187) -- characters two and three have tau fixed at 0 and are, bit for bit, what a call with tau=0 makes
    of them; and they match the reference's three-character call."""
    z = load_golden('albania_free_params')
    df = three_column_df(z)
    columns = list(z['three_columns'])
    tree, results = run_acr(df, model=F81, tau=None)
    assert [r['character'] for r in results] == columns
    assert results[0][MODEL]._optimise_tau and results[0][MODEL].tau == 0.0
    tree0, alone = run_acr(df[columns[1:]], model=F81, tau=0)
    for res, own, column in zip(results[1:], alone, columns[1:]):
        assert not res[MODEL]._optimise_tau and res[MODEL].tau == 0 and own[MODEL].tau == 0
        assert res[LOG_LIKELIHOOD] == own[LOG_LIKELIHOOD] and res[MODEL].sf == own[MODEL].sf
        assert np.array_equal(res[MODEL].frequencies, own[MODEL].frequencies)
        assert np.array_equal(res[MARGINAL_PROBABILITIES].values, own[MARGINAL_PROBABILITIES].values)
        assert np.array_equal(selected(tree, res, column)[1], selected(tree0, own, column)[1])

        def ref(key):
            return z['three_{}_{}'.format(column, key)]

        assert float(ref('tau')) == 0.0
        np.testing.assert_allclose(res[LOG_LIKELIHOOD], ref('loglik'), rtol=0, atol=2e-6)
        np.testing.assert_allclose(res[MODEL].sf, ref('sf'), rtol=2e-4)
        np.testing.assert_allclose(res[MODEL].frequencies, ref('frequencies'), rtol=0, atol=2e-5)
        np.testing.assert_allclose(res[MARGINAL_PROBABILITIES].values, ref('posterior'), rtol=0, atol=2e-5)
        np.testing.assert_allclose(res[RESTRICTED_LOG_LIKELIHOOD_FORMAT_STR.format(MPPA)], ref('loglik_restricted_MPPA'),
                                   rtol=0, atol=1e-4)


def branch_sum(flat, block, j):
    """G = sum of 1 / (1 - e_n) over the branches with e_n < 1 for point j of a block, in float64 with -expm1."""
    pi = block.pi[j]
    mu = 1. / (1. - pi.dot(pi))
    t = (flat.dist[flat.parent >= 0] + block.tau[j]) * block.tf[j] * block.sf[j]
    return float((1. / -np.expm1(-mu * t[t > 0])).sum())


def test_f81_with_free_tau_follows_the_reference_as_a_function():
    """
    Every vector the reference's objective was asked at during acr(F81, tau=None) -- 42 of (sf, tau) with the observed
    frequencies in place, 469 of (sf, tau, four frequency ratios) --, decoded in order by the model's kernel_points and
    evaluated in blocks of block_width(model) columns: each ln L within 2 tol of the value the reference returned,
    tol = LNL_RTOL |L| + 2^-53 G (both sides carry the rounding; tests/test_gpu_optimiser_points.py derives tol).
    """
    z = load_golden('albania_free_params')
    tree = read_tree(TREE_NWK)
    df = country_df()
    states = np.array(sorted(v for v in df[COUNTRY].unique() if not pd.isna(v) and '' != v))
    preannotate_forest([tree], df=df)
    stats = ForestStats([tree])
    flat = get_flat_forest([tree])
    _, observed, _ = calculate_observed_freqs(COUNTRY, [tree], states, flat)
    assert np.array_equal(observed, z['observed_frequencies'])
    model = F81Model(states=states, forest_stats=stats, tau=0, optimise_tau=True, observed_frequencies=observed,
                     character=COUNTRY)
    lengths, xs, values = z['F81_tau_trace_n'], z['F81_tau_trace_x'], -z['F81_tau_trace_value']
    n_basic = int((lengths == 2).sum())
    assert (lengths[:n_basic] == 2).all() and (lengths[n_basic:] == len(states) + 1).all() and n_basic and n_basic < len(lengths)
    width = block_width(model)
    assert width == len(states) + 2
    worst, first_out = 0.0, None
    with CharacterBatch(flat, len(states), 1) as batch:
        batch.set_annotation(0, *annotation_words(flat, COUNTRY, states))
        batch.initialize_allowed_states()
        batch.open_optimiser([width])
        for a, b, fixed in ((0, n_basic, True), (n_basic, len(lengths), False)):
            if fixed:   # (the first search: sf and tau alone, the frequencies at the observed ones, pastml/ml.py:216-218)
                model.fix_extra_params()
                model.frequencies = observed
            else:
                model.unfix_extra_params()
            for at in range(a, b, width):
                rows = slice(at, min(at + width, b))
                block = model.kernel_points(xs[rows, :lengths[at]])
                assert type(block) is PointBlock
                got = batch.evaluate_points({0: block})[0]
                assert not isinstance(got, LikelihoodError), got
                for j, (ours, theirs) in enumerate(zip(got, values[rows])):
                    tol = LNL_RTOL * abs(theirs) + 2.0 ** -53 * branch_sum(flat, block, j)
                    ratio = abs(ours - theirs) / (2 * tol)
                    if ratio >= 1 and first_out is None:
                        first_out = (at + j, xs[at + j], ours, theirs, tol)
                    worst = max(worst, ratio)
    print('worst |ours - reference| / (2 tol) over {} evaluations: {:.3g}'.format(len(values), worst))
    assert first_out is None, 'evaluation {} at {}: ln L {!r}, the reference returned {!r}, tol {:.3g}'.format(*first_out)


def test_f81_with_free_tau_ends_inside_the_references_own_range():
    z = load_golden('albania_free_params')
    tree, results = run_acr(country_df(), **run_kwargs(z, 'F81_tau'))
    res = results[0]
    theirs = [float(z['F81_tau_{}loglik'.format(r)]) for r in REPEATS]
    print('F81, tau free: ln L {!r}, sf {!r}, tau {!r}; the reference\'s three repeats: {}'
          .format(res[LOG_LIKELIHOOD], res[MODEL].sf, res[MODEL].tau, theirs))
    assert res[MODEL].tau == 0.0
    assert min(theirs) - 2e-6 <= res[LOG_LIKELIHOOD] <= max(theirs) + 2e-6
