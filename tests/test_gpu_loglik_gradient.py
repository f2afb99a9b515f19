"""
pml_loglik_gradient / Engine.loglik_gradient / ml.loglikelihood_gradient on the device against the decimal restatement of the
sums (tests/loglik_gradient_ref.py), bit-reproducibility over schedules, numberings, columns and calls, the count of flat
branches, and the refusals.

Error measure: |device - exact| / gross per component, the gross sums being those of the restatement (every term of a
component's sum replaced by a bound of its size).  TOLERANCE is 8 x the worst ratio seen on an MI355X over all the cases of this
file (room for another box's summation order), recorded in profiles/loglik_gradient.txt; it has to stay below 1e-11: a float64
restatement of these sums in numpy stays below 4e-16 of gross on such inputs, a dropped branch term or a wrong sign is 1e-3
of gross or more.
"""
import os

import numpy as np
import pandas as pd
import pytest

import loglik_gradient_cases as cases
import loglik_gradient_ref as gref
from conftest import load_golden, GOLDEN
from pastml_amd import hip, ml, synthetic
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.models.F81Model import F81Model
from pastml_amd.models.HKYModel import HKYModel
from pastml_amd.models.JCModel import JCModel
from pastml_amd.tree import FlatForest, read_tree

pytestmark = pytest.mark.gpu

TOLERANCE = 2.24e-13
assert TOLERANCE <= 1e-11

DATA = os.path.join(GOLDEN, 'data')
TREE_NWK = os.path.join(DATA, 'Albanian.tree.152tax.tre')
STATES_INPUT = os.path.join(DATA, 'data.txt')


def _model(kind, k, seed, tau):
    return dict(kind=hip.KIND_F81, pi=cases.frequencies(kind, k, seed)), cases.rates(seed, tau)


def _device(flat, masks_cols, models, k, tune=None, cols=None, calls=1):
    with hip.Engine(flat, len(models), k, tune=tune) as eng:
        eng.set_models(models)
        eng.set_masks(np.asarray(masks_cols))
        eng.marginal_pass(posterior=False, lh=False)
        for _ in range(calls):
            out = eng.loglik_gradient(*(cols or ()))
        return out


def _ratios(got, flat, masks, model, label):
    """The error ratios of one column's (d_rates [3], d_pi [k], n_flat) against the restatement; printed, then returned."""
    spec, (sf, tau, tf) = model
    g = gref.gradient(flat, masks, spec['pi'], sf, tau, tf)
    d_rates, d_pi, n_flat = got
    assert int(n_flat) == g['n_flat'], label
    assert np.isfinite(d_rates).all() and np.isfinite(d_pi).all(), label
    r = np.concatenate((gref.error_ratios(d_rates, [g['sf'], g['tau_fixed_tf'], g['tf']],
                                          [g['gross_sf'], g['gross_tau_fixed_tf'], g['gross_tf']]),
                        gref.error_ratios(d_pi, g['pi'], g['gross_pi'])))
    print('ratio {}: rates {:.3g} frequencies {:.3g}'.format(label, r[:3].max(), r[3:].max()))
    return r


def _check(got, flat, masks, model, label):
    r = _ratios(got, flat, masks, model, label)
    assert r.max() <= TOLERANCE, (label, r.max())


KS = (2, 3, 4, 5, 16, 17, 63, 64, 65, 130, 256, 257, 512)
CASES = [(kind, k) for kind in ('F81', 'JC') for k in KS]


@pytest.mark.parametrize('shape', cases.SHAPES)
@pytest.mark.parametrize('kind, k', CASES)
def test_device_against_the_reference(kind, k, shape):
    """Every shape at every k, F81 and JC, tau = 0 and tau > 0."""
    i = CASES.index((kind, k))
    flat = cases.forest(shape, seed=i % 3)
    masks = cases.masks(flat, k, i)
    for tau in (0.0, 0.011):
        model = _model(kind, k, i % 4, tau)
        d_rates, d_pi, n_flat = _device(flat, [masks], [model], k)
        if shape == 'zeros' and tau == 0:
            assert n_flat[0] > 0
        _check((d_rates[0], d_pi[0], n_flat[0]), flat, masks, model, '{} k={} {} tau={}'.format(kind, k, shape, tau))


@pytest.mark.parametrize('k', [5, 65])
def test_branches_of_1e_9_and_1e_12(k):
    flat = cases.forest('ragged')
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[3::7]] = 1e-9
    flat.dist[branches[5::7]] = 1e-12
    masks = cases.masks(flat, k, 2)
    model = _model('F81', k, 1, 0.0)
    d_rates, d_pi, n_flat = _device(flat, [masks], [model], k)
    assert n_flat[0] == 0
    _check((d_rates[0], d_pi[0], n_flat[0]), flat, masks, model, 'near-zero branches k={}'.format(k))


def test_n_flat_counts_the_branches_with_e_equal_to_one():
    flat = cases.forest('zeros')
    k = 4
    masks = cases.masks(flat, k, 0)
    n_zero = int((flat.dist[flat.parent >= 0] == 0).sum())
    assert n_zero > 0
    for tau, want in ((0.0, n_zero), (0.02, 0)):
        with hip.Engine(flat, 1, k) as eng:
            eng.set_models([_model('F81', k, 0, tau)])
            eng.set_masks(np.asarray([masks]))
            eng.marginal_pass(posterior=False, lh=False)
            n_flat = eng.loglik_gradient()[2]
            e = eng.download(hip.BUF_BRANCH_EXP, 0)
        assert n_flat[0] == int((e[flat.parent >= 0] == 1.0).sum()) == want


def _annotated(flat, k, seed):
    roots = flat.to_tree_nodes()
    states = synthetic.state_names(k)
    rng = np.random.default_rng(seed)
    for j, t in enumerate(flat.tips):
        if j % 10 != 3 and flat.dist[t] > 0:
            flat.nodes[t].add_feature('c', {states[rng.integers(0, k)]})
    return roots, states


def test_front_end_reports_tau_as_nan_exactly_where_branches_are_flat():
    k = 4
    for shape, tau, flat_expected in (('zeros', 0.0, True), ('zeros', 0.02, False), ('polytomy', 0.0, False)):
        flat = cases.forest(shape)
        roots, states = _annotated(flat, k, 1)
        model = F81Model(states=states, forest_stats=ForestStats(roots), sf=1.5, tau=tau, optimise_tau=True,
                         frequencies=cases.frequencies('F81', k, 0))
        out = ml.loglikelihood_gradient(roots, 'c', model)
        assert (out['n_zero_length_branches'] > 0) == flat_expected
        assert out['parameter_names'][:2] == ['scaling_factor', 'smoothing_factor']
        assert len(out['parameters']) == len(model.get_optimised_parameters()) == k + 1
        assert np.isnan(out['tau']) == flat_expected and np.isnan(out['parameters'][1]) == flat_expected
        assert np.isfinite(out['sf']) and np.isfinite(out['frequencies']).all() and np.isfinite(out['log_likelihood'])
        assert np.isfinite(np.delete(out['parameters'], 1)).all()


def test_front_end_with_frequency_smoothing_gives_the_natural_derivatives_only():
    k = 4
    flat = cases.forest('polytomy')
    roots, states = _annotated(flat, k, 1)
    pi = cases.frequencies('F81', k, 0)
    plain = ml.loglikelihood_gradient(roots, 'c', F81Model(states=states, forest_stats=ForestStats(roots), sf=1.5, frequencies=pi))
    out = ml.loglikelihood_gradient(roots, 'c', F81Model(states=states, forest_stats=ForestStats(roots), sf=1.5, frequencies=pi,
                                                         frequency_smoothing=True))
    assert out['parameters'] is None and out['parameter_names'] is None
    assert out['sf'] == plain['sf'] and np.array_equal(out['frequencies'], plain['frequencies'])


@pytest.mark.parametrize('k', [4, 16, 65])
def test_more_nodes_than_one_piece(k):
    """2 x piece + 37 nodes, once per piece size of the launcher (1024, 512 and 256 ids)."""
    piece = {4: 1024, 16: 512, 65: 256}[k]   # (gradient_piece, pml_launch_gradient.hip)
    flat = FlatForest.random(piece + 19, seed=21, max_arity=2, zero_frac=0.0, n_trees=1)
    assert flat.n_nodes == 2 * piece + 37
    masks = cases.masks(flat, k, 3)
    model = _model('F81', k, 2, 0.0)
    d_rates, d_pi, n_flat = _device(flat, [masks], [model], k)
    _check((d_rates[0], d_pi[0], n_flat[0]), flat, masks, model, 'pieces k={}'.format(k))


@pytest.mark.parametrize('k', [5, 24, 70])
def test_several_columns_with_their_own_parameters(k):
    flat = cases.forest('forest')
    models = [_model('F81', k, s, 0.01 * (s % 3)) for s in range(5)]
    masks = [cases.masks(flat, k, 10 + s) for s in range(5)]
    d_rates, d_pi, n_flat = _device(flat, masks, models, k)
    for c in range(5):
        _check((d_rates[c], d_pi[c], n_flat[c]), flat, masks[c], models[c], 'k={} column {}'.format(k, c))
    # a sub-range of the columns is the same columns
    sub = _device(flat, masks, models, k, cols=(1, 4))
    assert np.array_equal(sub[0], d_rates[1:4]) and np.array_equal(sub[1], d_pi[1:4]) and np.array_equal(sub[2], n_flat[1:4])


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('k, n_tips', [(4, 3000), (24, 1500), (130, 700)])
def test_bits_do_not_depend_on_schedules_numbering_column_or_call(k, n_tips):
    flat = FlatForest.random(n_tips, seed=11, max_arity=3, zero_frac=0.0, n_trees=2)
    masks = cases.masks(flat, k, 1)
    model = _model('F81', k, 1, 0.0)
    base = _device(flat, [masks], [model], k)
    assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all()
    assert _same(base, _device(flat, [masks], [model], k, calls=2))
    assert _same(base, _device(flat, [masks], [model], k, tune={'NO_SUPER': 1}))
    assert _same(base, _device(flat, [masks], [model], k, tune={'NO_HEIGHT_ORDER': 1}))   # (the caller's numbering kept)
    others = [cases.masks(flat, k, 50 + c) for c in range(6)]
    other_models = [_model('F81', k, c % 4, 0.01 * (c % 2)) for c in range(6)]
    first = _device(flat, [masks] + others, [model] + other_models, k)
    last = _device(flat, others + [masks], other_models + [model], k)
    assert _same([x[0] for x in first], [x[0] for x in base])
    assert _same([x[6] for x in last], [x[0] for x in base])
    assert _same([x[1:] for x in first], [x[:6] for x in last])


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------

def _refused(eng, status, *words):
    with pytest.raises(hip.HipError) as info:
        eng.loglik_gradient()
    assert info.value.status == status, str(info.value)
    for word in words:
        assert word in str(info.value), str(info.value)


def test_refusals_leave_the_context_answering():
    flat = cases.forest('balanced')
    # no marginal pass
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([_model('F81', 4, 0, 0.0)])
        eng.set_masks(np.asarray([cases.masks(flat, 4, 0)]))
        _refused(eng, hip.PML_ERR_INVALID, 'pml_loglik_gradient', 'marginal')
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts()
        assert np.isfinite(counts).all()
        assert np.isfinite(eng.loglik_gradient()[0]).all()
        assert np.array_equal(eng.expected_counts(), counts)   # (the results of the pass stay)
    # a model kind other than F81
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([(dict(kind=hip.KIND_HKY, pi=cases.frequencies('F81', 4, 0), kappa=2.0), cases.rates(0, 0.0))])
        eng.set_masks(np.asarray([cases.masks(flat, 4, 0)]))
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, hip.PML_ERR_UNSUPPORTED, 'F81', 'HKY')
        assert np.isfinite(eng.expected_counts()).all()
    # a column whose pi . pi is 1: mu is infinite (every tip in the one state there is, or missing)
    with hip.Engine(flat, 2, 2) as eng:
        eng.set_models([_model('F81', 2, 0, 0.0), (dict(kind=hip.KIND_F81, pi=np.array([1.0, 0.0])), cases.rates(0, 0.0))])
        masks = np.ones((2, flat.n_nodes, 2), dtype=np.int8)
        masks[:, flat.tips[::2], 1] = 0
        eng.set_masks(masks)
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, hip.PML_ERR_INVALID, 'column 1', 'pi . pi')
        assert np.isfinite(eng.loglik_gradient(0, 1)[0]).all()   # (the other column is served)
        assert np.isfinite(eng.expected_counts(0, 1)).all()
    # one state
    with hip.Engine(flat, 1, 1) as eng:
        eng.set_models([(dict(kind=hip.KIND_F81, pi=np.array([1.0])), cases.rates(0, 0.0))])
        eng.set_masks(np.ones((1, flat.n_nodes, 1), dtype=np.int8))
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, hip.PML_ERR_INVALID, 'k = 1')
        assert np.isfinite(eng.expected_counts()).all()


def test_front_end_refuses_other_models_by_name():
    flat = cases.forest('balanced')
    roots = flat.to_tree_nodes()
    model = HKYModel(forest_stats=ForestStats(roots), sf=1.0)
    with pytest.raises(NotImplementedError, match='HKY'):
        ml.loglikelihood_gradient(roots, 'c', model)


# ---------------------------------------------------------------------------------------------------------------------
# the front end on the Albania tree
# ---------------------------------------------------------------------------------------------------------------------

def _albania():
    zz = load_golden('albania_F81')
    tree = read_tree(TREE_NWK)
    preannotate_forest([tree], df=pd.read_csv(STATES_INPUT, index_col=0, header=0)[['Country']])
    return tree, zz


def _host_view(tree, model):
    """(flat, masks the marginal pass runs with: altered where tau == 0)"""
    problem = ml.ForestProblem([tree], 'Country', model.states)
    problem.initialize_allowed_states()
    if 0 == model.tau:
        problem.alter_zero_node_allowed_states()
    return problem.flat, problem.masks.astype(int)


def test_front_end_on_the_albania_tree():
    tree, zz = _albania()
    stats = ForestStats([tree])
    f81 = F81Model(states=zz['opt_states'], forest_stats=stats, sf=float(zz['opt_sf']), frequencies=zz['opt_frequencies'])
    jc = JCModel(states=zz['opt_states'], forest_stats=stats, sf=float(zz['opt_sf']))
    k = len(f81.states)
    out = ml.loglikelihood_gradient([tree], 'Country', f81)
    assert len(out['parameters']) == k and len(out['parameter_names']) == k and out['parameter_names'][0] == 'scaling_factor'
    both = ml.loglikelihood_gradient([tree], ['Country', 'Country'], [f81, jc])
    assert np.array_equal(both[0]['parameters'], out['parameters']) and both[0]['log_likelihood'] == out['log_likelihood']
    assert both[1]['parameter_names'] == ['scaling_factor'] and len(both[1]['parameters']) == 1
    for model, result, label in ((f81, out, 'Albania F81'), (jc, both[1], 'Albania JC')):
        flat, masks = _host_view(tree, model)
        sf, tau, tf = model.rate_params()
        g = gref.gradient(flat, masks, model.frequencies, sf, tau, tf)
        assert result['n_zero_length_branches'] == g['n_flat'] > 0 and np.isnan(result['tau'])
        assert abs(result['log_likelihood'] - float(g['loglik'])) < 1e-9 * abs(float(g['loglik']))
        want, gross = gref.chain_rule(g, model.frequencies, tau, stats.forest_length, stats.num_nodes, free_sf=True,
                                      free_tau=False, free_frequencies=model is f81)
        r = gref.error_ratios(result['parameters'], want, gross)
        print('ratio {}: parameters {:.3g}'.format(label, r.max()))
        print('{}: gradient at the stored parameters {}'.format(label, dict(zip(result['parameter_names'], result['parameters']))))
        assert r.max() <= TOLERANCE, (label, r.max())
        natural = gref.error_ratios(np.concatenate(([result['sf']], result['frequencies'])), [g['sf']] + g['pi'],
                                    [g['gross_sf']] + g['gross_pi'])
        assert natural.max() <= TOLERANCE, (label, natural.max())
