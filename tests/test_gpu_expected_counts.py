"""
pml_expected_counts / ml.expected_counts / count_transitions on the device against the numpy restatement of the definition
(tests/expected_counts_ref.py, on the oracle's sweeps), bit-reproducibility over schedules, numberings and columns, the
sampler within its own noise, and one run at full size.

Tolerance of the comparisons with the restatement: the project's posterior tolerance, 1e-9 relative per entry; on the diagonal,
where the correction subtracts terms of the size of the sum, an absolute floor of 1e-9 x (number of branches).
"""
import os

import numpy as np
import pandas as pd
import pytest

import expected_counts_ref as xref
from conftest import load_golden, GOLDEN
from oracle import pastml_oracle as orc
from pastml_amd import hip, ml, synthetic
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.models.F81Model import F81Model, F81
from pastml_amd.models.JCModel import JCModel, JC
from pastml_amd.tree import FlatForest, read_tree

pytestmark = pytest.mark.gpu

DATA = os.path.join(GOLDEN, 'data')
TREE_NWK = os.path.join(DATA, 'Albanian.tree.152tax.tre')
STATES_INPUT = os.path.join(DATA, 'data.txt')
PARAMS_F81 = os.path.join(DATA, 'albania_pastml', 'params.character_Country.method_MPPA.model_F81.tab')


def _forest(shape, seed=0):
    if shape == 'balanced':
        return synthetic.balanced_forest(5)
    if shape == 'ragged':
        return FlatForest.random(45, seed=3 + seed, max_arity=2, zero_frac=0.0, n_trees=1)
    if shape == 'polytomy':
        return FlatForest.random(50, seed=5 + seed, max_arity=5, zero_frac=0.0, n_trees=1)
    if shape == 'forest':
        return FlatForest.random(60, seed=7 + seed, max_arity=4, zero_frac=0.0, n_trees=3)
    raise ValueError(shape)


def _masks(flat, k, seed):
    """one-hot tips, some missing (all ones), some with two states"""
    rng = np.random.default_rng(100 + seed)
    masks = np.ones((flat.n_nodes, k), dtype=np.int8)
    tips = flat.tips
    masks[tips] = 0
    masks[tips, rng.integers(0, k, size=len(tips))] = 1
    masks[tips[::9]] = 1
    for t in tips[4::11]:
        masks[t, rng.integers(0, k)] = 1
    return masks


def _spec(kind, k, seed):
    rng = np.random.default_rng(1000 + 17 * k + seed)
    rates = (0.7 + 0.4 * seed, 0.01 * (seed % 3), 1.0 - 0.05 * (seed % 2))
    if kind == 'F81':
        return dict(kind=hip.KIND_F81, pi=rng.dirichlet(np.ones(k) * 2)), rates
    if kind == 'JC':
        return dict(kind=hip.KIND_F81, pi=np.full(k, 1.0 / k)), rates
    if kind == 'HKY':
        return dict(kind=hip.KIND_HKY, pi=rng.dirichlet(np.ones(4) * 3), kappa=2.0 + seed), rates
    pi = rng.dirichlet(np.ones(k) * 3)
    r = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
    d, a, ainv = orc.diagonalise(pi, r + r.T)
    return dict(kind=hip.KIND_EIGEN, pi=pi, d=d, A=a, Ainv=ainv), rates


def _assert_close(got, want, n_branches, label):
    k = want.shape[0]
    off = ~np.eye(k, dtype=bool)
    err = np.abs(got - want)
    rel = err[off] / np.maximum(np.abs(want[off]), 1e-300)
    print('{}: max rel off-diagonal {:.3g}, max abs diagonal {:.3g}'.format(label, rel.max() if rel.size else 0.0,
                                                                            err[~off].max()))
    np.testing.assert_allclose(got[off], want[off], rtol=1e-9, atol=1e-300, err_msg=label)
    np.testing.assert_allclose(got[~off], want[~off], rtol=1e-9, atol=1e-9 * n_branches, err_msg=label)


def _restated(flat, masks, spec, rates):
    return xref.from_oracle(orc, flat, masks.astype(int), spec, sf=rates[0], tau=rates[1], tf=rates[2])


def _device(flat, masks_cols, models, k, tune=None, options=()):
    with hip.Engine(flat, len(models), k, tune=tune) as eng:
        for opt, value in options:
            eng.set_option(opt, value)
        eng.set_models(models)
        eng.set_masks(np.asarray(masks_cols))
        eng.marginal_pass(posterior=False, lh=False)
        return eng.expected_counts()


CASES = [('F81', k) for k in (2, 4, 5, 15, 16, 17, 63, 64, 65, 130, 256, 257, 300, 512)] + [('JC', 4), ('HKY', 4)] + \
        [('CR', k) for k in (2, 5, 20, 61, 100, 200)]
SHAPES = ['balanced', 'ragged', 'polytomy', 'forest']


@pytest.mark.parametrize('kind, k', CASES)
def test_device_against_the_restatement(kind, k):
    i = CASES.index((kind, k))
    shapes = SHAPES if k <= 20 else [SHAPES[i % 4], SHAPES[(i + 1) % 4]]
    for shape in shapes:
        flat = _forest(shape, seed=i % 3)
        masks = _masks(flat, k, i)
        spec, rates = _spec(kind, k, i % 4)
        got = _device(flat, [masks], [(spec, rates)], k)[0]
        want = _restated(flat, masks, spec, rates)
        assert not np.isnan(got).any()
        _assert_close(got, want['counts'], flat.n_nodes - len(flat.roots), '{} k={} {}'.format(kind, k, shape))


@pytest.mark.parametrize('kind, k', [('F81', 5), ('F81', 24), ('F81', 70), ('HKY', 4), ('CR', 20), ('CR', 70)])
def test_several_columns_with_their_own_parameters(kind, k):
    flat = _forest('forest')
    models = [_spec(kind, k, s) for s in range(5)]
    masks = [_masks(flat, k, 10 + s) for s in range(5)]
    got = _device(flat, masks, models, k)
    for c in range(5):
        want = _restated(flat, masks[c], *models[c])
        _assert_close(got[c], want['counts'], flat.n_nodes - len(flat.roots), '{} k={} column {}'.format(kind, k, c))
    # a sub-range of the columns is the same columns
    with hip.Engine(flat, 5, k) as eng:
        eng.set_models(models)
        eng.set_masks(np.asarray(masks))
        eng.marginal_pass(posterior=False, lh=False)
        assert np.array_equal(eng.expected_counts(1, 4), got[1:4])


def test_needs_a_marginal_pass():
    flat = _forest('balanced')
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([_spec('F81', 4, 0)])
        eng.set_masks(np.asarray([_masks(flat, 4, 0)]))
        with pytest.raises(hip.HipError):
            eng.expected_counts()


# ---------------------------------------------------------------------------------------------------------------------
# altered forests through ml.expected_counts
# ---------------------------------------------------------------------------------------------------------------------

def _annotated_zero_forest(k, seed, n_tips=70):
    flat = FlatForest.random(n_tips, seed=seed, max_arity=3, zero_frac=0.3, n_trees=2)
    roots = flat.to_tree_nodes()
    states = synthetic.state_names(k)
    rng = np.random.default_rng(seed)
    for j, t in enumerate(flat.tips):
        if j % 10 != 3:
            flat.nodes[t].add_feature('c', {states[rng.integers(0, k)]})
    return flat, roots, states


def _host_masks(roots, model):
    problem = ml.ForestProblem(roots, 'c', model.states)
    problem.initialize_allowed_states()
    altered = np.zeros(problem.N, dtype=bool)
    if 0 == model.tau:
        altered[problem.alter_zero_node_allowed_states()] = True
    return problem.flat, problem.masks.astype(int), altered, problem.init_masks.astype(int)


@pytest.mark.parametrize('k, seed', [(3, 1), (4, 2), (20, 3)])
def test_altered_forests_through_ml_expected_counts(k, seed):
    flat, roots, states = _annotated_zero_forest(k, seed)
    rng = np.random.default_rng(seed)
    model = F81Model(states=states, forest_stats=ForestStats(roots), sf=1.5, frequencies=rng.dirichlet(np.ones(k) * 3))
    model.freeze()
    pflat, masks, altered, initial = _host_masks(roots, model)
    assert altered.any(), 'the case must have altered nodes'
    spec = dict(kind=orc.KIND_F81, pi=np.asarray(model.frequencies, dtype=np.float64))
    sf, tau, tf = model.rate_params()
    want = xref.from_oracle(orc, pflat, masks, spec, sf=sf, tau=tau, tf=tf, altered=altered, initial=initial)
    got = ml.expected_counts(roots, 'c', model)
    _assert_close(got, want['counts'], pflat.n_nodes - len(pflat.roots), 'altered k={}'.format(k))
    # a list of characters: the same arrays
    again = ml.expected_counts(roots, ['c', 'c'], [model, model])
    assert np.array_equal(again[0], got) and np.array_equal(again[1], got)


def test_tau_positive_takes_the_plain_path():
    flat, roots, states = _annotated_zero_forest(4, 2)
    model = JCModel(states=states, forest_stats=ForestStats(roots), sf=1.5, tau=0.02)
    model.freeze()
    seen = []
    real = hip.Engine.expected_counts

    def spy(self, col_begin=0, col_end=None, altered=None):
        seen.append(altered is not None)
        return real(self, col_begin, col_end, altered=altered)

    hip.Engine.expected_counts = spy
    try:
        got = ml.expected_counts(roots, 'c', model)
    finally:
        hip.Engine.expected_counts = real
    assert seen == [False]
    pflat, masks, altered, initial = _host_masks(roots, model)
    assert not altered.any()
    spec = dict(kind=orc.KIND_F81, pi=np.asarray(model.frequencies, dtype=np.float64))
    sf, tau, tf = model.rate_params()
    want = xref.from_oracle(orc, pflat, masks, spec, sf=sf, tau=tau, tf=tf)
    _assert_close(got, want['counts'], pflat.n_nodes - len(pflat.roots), 'tau > 0')


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind, k, shape', [('F81', 24, 'big_balanced'), ('F81', 24, 'big_ragged'), ('F81', 4, 'big_ragged'),
                                            ('CR', 20, 'mid_ragged')])
def test_bits_do_not_depend_on_schedules_numbering_or_column(kind, k, shape):
    if shape == 'big_balanced':
        flat = synthetic.balanced_forest(15)
    elif shape == 'big_ragged':
        flat = FlatForest.random(40000, seed=11, max_arity=2, zero_frac=0.0, n_trees=1)
    else:
        flat = FlatForest.random(3000, seed=12, max_arity=3, zero_frac=0.0, n_trees=2)
    masks = _masks(flat, k, 1)
    model = _spec(kind, k, 1)
    base = _device(flat, [masks], [model], k)[0]
    assert np.isfinite(base).all()
    assert np.array_equal(base, _device(flat, [masks], [model], k)[0])
    assert np.array_equal(base, _device(flat, [masks], [model], k, tune={'NO_SUPER': 1})[0])
    assert np.array_equal(base, _device(flat, [masks], [model], k, tune={'NO_HEIGHT_ORDER': 1})[0])
    if kind == 'F81':
        assert np.array_equal(base, _device(flat, [masks], [model], k,
                                            options=[(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)])[0])
    # the character in column 0 or in column 31 of a batch of other characters
    others = [_masks(flat, k, 50 + c) for c in range(31)]
    other_models = [_spec(kind, k, c % 4) for c in range(31)]
    first = _device(flat, [masks] + others, [model] + other_models, k)
    last = _device(flat, others + [masks], other_models + [model], k)
    assert np.array_equal(first[0], base)
    assert np.array_equal(last[31], base)
    assert np.array_equal(first[1:], last[:31])


# ---------------------------------------------------------------------------------------------------------------------
# against the sampler, and the file-level front end
# ---------------------------------------------------------------------------------------------------------------------

def _bound(ref, n_rep, extra):
    return 6 * np.sqrt(np.maximum(ref, 0.05) / n_rep) * 3 + extra


def _albania_model():
    zz = load_golden('albania_F81')
    tree = read_tree(TREE_NWK)
    preannotate_forest([tree], df=pd.read_csv(STATES_INPUT, index_col=0, header=0)[['Country']])
    model = F81Model(states=zz['opt_states'], forest_stats=ForestStats([tree]), sf=float(zz['opt_sf']),
                     frequencies=zz['opt_frequencies'])
    model.freeze()
    return tree, model


def test_sampler_within_its_noise_of_the_exact_counts():
    z = load_golden('marginal_counts')
    n_rep = 40000
    np.random.seed(7)
    flat = synthetic.balanced_forest(6)
    roots = flat.to_tree_nodes()
    states = synthetic.state_names(4)
    for j, t in enumerate(flat.tips):
        flat.nodes[t].add_feature('c', {states[z['jc_tip_states'][j]]})
    model = JCModel(states=states, forest_stats=ForestStats(roots), sf=float(z['jc_sf']))
    model.freeze()
    exact = ml.expected_counts(roots, 'c', model)
    sampled = ml.marginal_counts(roots, 'c', model, n_repetitions=n_rep)
    diff = np.abs(sampled - exact)
    print('JC: max |sampler - exact| =', diff.max())
    assert np.all(diff < _bound(exact, n_rep, 0.02)), diff.max()
    # ... and of the reference's own estimate
    assert np.all(np.abs(z['jc_counts'] - exact) < _bound(z['jc_counts'], n_rep, 0.02))

    tree, model = _albania_model()
    exact = ml.expected_counts([tree], 'Country', model)
    sampled = ml.marginal_counts([tree], 'Country', model, n_repetitions=n_rep)
    diff = np.abs(sampled - exact)
    print('Albania: max |sampler - exact| =', diff.max())
    assert np.all(diff < _bound(exact, n_rep, 0.03)), (diff.max(), sampled.round(3), exact.round(3))
    assert np.all(np.abs(z['albania_counts'] - exact) < _bound(z['albania_counts'], n_rep, 0.03))


def test_count_transitions_on_the_albania_files(tmp_path):
    from pastml_amd.utilities.transition_counter import count_transitions
    out = str(tmp_path / 'exact.tab')
    count_transitions(TREE_NWK, STATES_INPUT, 'Country', PARAMS_F81, out, data_sep=',', model=F81, n_repetitions=None)
    table = pd.read_csv(out, sep='\t', index_col=0)
    assert table.index.name == 'from'
    # the same model as the front end builds, through ml.expected_counts
    from pastml_amd.pipeline import validate_input
    from pastml_amd.acr import calculate_observed_freqs
    forest, columns, column2states, parameters, _ = validate_input(TREE_NWK, ['Country'], STATES_INPUT, ',', 0,
                                                                   parameters=[PARAMS_F81])
    states = column2states['Country']
    assert list(table.index) == list(states) == list(table.columns)
    _, freqs, _ = calculate_observed_freqs('Country', forest, states)
    model = F81Model(parameter_file=PARAMS_F81, reoptimise=False, states=states, forest_stats=ForestStats(forest),
                     observed_frequencies=freqs)
    exact = ml.expected_counts(forest, 'Country', model)
    np.testing.assert_allclose(table.values, exact, rtol=1e-12, atol=1e-15)   # (the table is written with repr precision)
    # the sampled table with the reference's default number of repetitions, within its own standard error
    np.random.seed(3)
    sampled_path = str(tmp_path / 'sampled.tab')
    count_transitions(TREE_NWK, STATES_INPUT, 'Country', PARAMS_F81, sampled_path, data_sep=',', model=F81,
                      n_repetitions=1000)
    sampled = pd.read_csv(sampled_path, sep='\t', index_col=0).values
    diff = np.abs(sampled - exact)
    print('count_transitions: max |1000 repetitions - exact| =', diff.max())
    assert np.all(diff < _bound(exact, 1000, 0.03)), diff.max()
    # two columns through the template: two files
    df = pd.read_csv(STATES_INPUT, index_col=0, header=0)
    df['Region'] = df['Country'].replace({'Albania': 'Greece'})
    two = str(tmp_path / 'two.csv')
    df.to_csv(two)
    template = str(tmp_path / 'counts.{column}.tab')
    count_transitions(TREE_NWK, two, ['Country', 'Region'], {'Country': PARAMS_F81, 'Region': {'scaling_factor': 2.0}},
                      template, data_sep=',', model=F81, n_repetitions=None)
    first = pd.read_csv(str(tmp_path / 'counts.Country.tab'), sep='\t', index_col=0)
    second = pd.read_csv(str(tmp_path / 'counts.Region.tab'), sep='\t', index_col=0)
    np.testing.assert_allclose(first.values, exact, rtol=1e-12, atol=1e-15)
    assert second.shape == (4, 4) and np.isfinite(second.values).all()


# ---------------------------------------------------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------------------------------------------------

def test_full_size_one_call():
    """262 144 tips x 32 columns (every column its own parameters), k = 64, one call, and the row-sum identity on every column:
    every row of M_n sums to one, so sum_b counts[a][b] + sum_p min(q_p[a], same_p[a]) = sum over the branches of q_parent[a].
    same_p[a] = sum over the children of q_p[a] w_n[a] ((1 - e) pi_a + e) / den_n[a] is formed here in numpy, vectorised over
    the nodes, from the column's downloaded bottom-up vectors, posteriors and branch exponentials.  1e-9 relative."""
    import time
    L, k, C = 18, 64, 32
    flat = synthetic.balanced_forest(L)
    N = flat.n_nodes
    n_internal = int((flat.n_children > 0).sum())
    # level order of a balanced binary tree: the children of p are 2 p + 1 and 2 p + 2
    assert np.array_equal(flat.first_child[:n_internal], 2 * np.arange(n_internal) + 1)
    assert np.all(flat.n_children[:n_internal] == 2) and np.all(flat.n_children[n_internal:] == 0)
    parent = flat.parent[1:]
    rng = np.random.default_rng(0)
    states = rng.integers(0, k, size=(C, len(flat.tips))).astype(np.int32)
    states[:, ::17] = -1   # missing tips
    models = [_spec('F81', k, c) for c in range(C)]
    with hip.Engine(flat, C, k) as eng:
        eng.set_models(models)
        eng.set_tip_states(states)
        eng.marginal_pass(posterior=False, lh=False)
        t0 = time.time()
        counts = eng.expected_counts()
        print('full size: {:.3f} s for the call'.format(time.time() - t0))
        assert counts.shape == (C, k, k) and np.isfinite(counts).all()
        worst = 0.0
        for c in range(C):
            pi = models[c][0]['pi']
            post = eng.download(hip.BUF_POSTERIOR, c)
            w = eng.download(hip.BUF_BU, c)[1:]    # (tips: their masks as 0/1; the internal nodes' masks are all ones)
            w *= pi
            e = eng.download(hip.BUF_BRANCH_EXP, c)[1:, None]
            qp = post[parent]
            den = (1.0 - e) * pi * w.sum(axis=1, keepdims=True) + e * w
            used = (qp > 0) & (den > 0)
            term = np.where(used, qp * w * ((1.0 - e) * pi + e) / np.where(used, den, 1.0), 0.0)
            same = term.reshape(n_internal, 2, k).sum(axis=1)
            correction = np.minimum(post[:n_internal], same).sum(axis=0)
            mass = np.where(used, qp, 0.0).sum(axis=0)
            lhs = counts[c].sum(axis=1) + correction
            rel = np.abs(lhs - mass) / mass
            worst = max(worst, rel.max())
            assert np.all(rel < 1e-9), (c, rel.max())
            assert np.all(counts[c] >= -1e-9 * N), c
        print('full size: row-sum identity, max relative deviation over the columns {:.3g}'.format(worst))


def test_marginal_counts_restricts_to_initial_states_when_no_draw_hits_them():
    """The sampler's to_initial fallback (ml.py:806-812: an altered node none of whose draws fell on the states it had gets
    those states evenly) with few repetitions on Albania, where an altered zero-length tip's posterior sits on another state:
    the device path and the host path.  The masks are int8 arrays; n_repetitions times them must not be formed in int8."""
    tree, model = _albania_model()
    for n_rep in (200, 1000):
        for device_sampling in (True, False):
            np.random.seed(11)
            got = ml.marginal_counts([tree], 'Country', model, n_repetitions=n_rep, device_sampling=device_sampling)
            assert np.isfinite(got).all() and np.all(got >= -1e-12)
            exact = ml.expected_counts([tree], 'Country', model)
            assert np.all(np.abs(got - exact) < _bound(exact, n_rep, 0.03))
