"""Forward simulation of a character on the device (pastml_amd.utilities.state_simulator, pml_simulate_states)."""
import os

import numpy as np
import pandas as pd
import pytest
from scipy import stats

from conftest import GOLDEN, load_golden
from sampler_ref import ALPHA, _check_transitions
from pastml_amd import hip, ml
from pastml_amd.acr import acr
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.ml import LOG_LIKELIHOOD, MARGINAL_PROBABILITIES, MODEL, MPPA
from pastml_amd.models.CustomRatesModel import CUSTOM_RATES
from pastml_amd.models.F81Model import F81
from pastml_amd.models.JTTModel import JTT, JTT_RATE_MATRIX, JTT_STATES
from pastml_amd.models.generator import save_matrix
from pastml_amd.models._closed_form import EFTModel, F81Model, HKYModel, JCModel
from pastml_amd.models._eigen import CustomRatesModel, JTTModel
from pastml_amd.tree import FlatForest, read_tree
from pastml_amd.utilities.state_simulator import simulate_states

DATA = os.path.join(GOLDEN, 'data')


def _forest(flat):
    roots = flat.to_tree_nodes()
    return roots, flat


def _random_forest():
    flat = FlatForest.random(60, seed=3, max_arity=4, zero_frac=0.15, n_trees=3)
    roots, flat = _forest(flat)
    return roots, flat


def _model(kind, k, roots, sf=1.7, tau=0.0):
    fs = ForestStats(roots)
    rng = np.random.default_rng(k)
    if kind == 'F81':
        pi = rng.dirichlet(np.ones(k) * 2)
        return F81Model(states=np.array(['s{}'.format(i) for i in range(k)]), forest_stats=fs, sf=sf, tau=tau, frequencies=pi)
    if kind == 'JC':
        return JCModel(states=np.array(['s{}'.format(i) for i in range(k)]), forest_stats=fs, sf=sf, tau=tau)
    if kind == 'EFT':
        pi = rng.dirichlet(np.ones(k) * 2)
        return EFTModel(states=np.array(['s{}'.format(i) for i in range(k)]), forest_stats=fs, observed_frequencies=pi, sf=sf,
                        tau=tau)
    if kind == 'HKY':
        return HKYModel(forest_stats=fs, sf=sf, tau=tau, kappa=3.0, frequencies=np.array([0.4, 0.1, 0.2, 0.3]))
    if kind == 'JTT':
        return JTTModel(forest_stats=fs, sf=sf, tau=tau)
    if kind == 'CR5':
        return CustomRatesModel(forest_stats=fs, sf=sf, tau=tau, states=np.array(['s{}'.format(i) for i in range(5)]),
                                rate_matrix_file=os.path.join(DATA, 'custom_rates_k5.txt'))
    if kind == 'CR':
        rates = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
        return CustomRatesModel(forest_stats=fs, sf=sf, tau=tau, states=np.array(['s{}'.format(i) for i in range(k)]),
                                rate_matrix=rates + rates.T, frequencies=rng.dirichlet(np.ones(k) * 3))
    raise ValueError(kind)


CASES = [('F81', 5, 0.0, 4000), ('F81', 64, 0.0, 20000), ('F81', 300, 0.3, 20000), ('JC', 4, 0.0, 4000),
         ('EFT', 6, 0.2, 4000), ('HKY', 4, 0.0, 4000), ('JTT', 20, 0.1, 8000), ('CR5', 5, 0.0, 4000), ('CR', 100, 0.0, 20000),
         ('CR', 200, 0.1, 20000)]   # (beyond 128 states the cumulative rows live in a scratch buffer)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,k,tau,n_rep', CASES, ids=['{}-k{}'.format(c[0], c[1]) for c in CASES])
def test_transition_frequencies_follow_pij(kind, k, tau, n_rep):
    roots, flat = _random_forest()
    model = _model(kind, k, roots, tau=tau)
    k = len(model.states)
    np.random.seed(7)
    simulate_states(roots, model, 'sim', n_repetitions=n_rep)
    sim = np.stack([flat.nodes[i].sim for i in range(flat.n_nodes)])
    assert sim.shape == (flat.n_nodes, n_rep)
    assert sim.dtype == (np.uint8 if k <= 256 else np.uint16)
    assert int(sim.max()) < k
    _check_transitions(flat, model, sim, k)


@pytest.mark.gpu
def test_deep_caterpillar():
    depth = 2000
    n = 2 * depth + 1
    parent = np.full(n, -1, dtype=np.int32)
    n_children = np.zeros(n, dtype=np.int32)
    first_child = np.zeros(n, dtype=np.int32)
    # breadth-first ids: the spine node of depth d is 2d - 1 (d >= 1; the root is 0), its tip sibling 2d
    spine = [0] + [2 * d - 1 for d in range(1, depth + 1)]
    for d in range(depth):
        p = spine[d]
        n_children[p] = 2
        first_child[p] = 2 * d + 1
        parent[2 * d + 1] = p
        parent[2 * d + 2] = p
    dist = np.random.default_rng(5).uniform(0.001, 0.2, size=n)
    flat = FlatForest(parent, n_children, first_child, dist, np.array([0]))
    assert flat.n_td_levels == depth + 1
    roots, flat = _forest(flat)
    model = _model('F81', 4, roots, sf=2.0)
    np.random.seed(11)
    simulate_states(roots, model, 'sim', n_repetitions=2000)
    sim = np.stack([flat.nodes[i].sim for i in range(flat.n_nodes)])
    _check_transitions(flat, model, sim, 4)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,k', [('F81', 6), ('JC', 4), ('EFT', 5)])
def test_zero_branches_copy_the_parent(kind, k):
    roots, flat = _random_forest()
    zero = np.flatnonzero((flat.dist == 0) & (flat.parent >= 0))
    assert len(zero) > 3
    model = _model(kind, k, roots, tau=0.0)
    np.random.seed(3)
    simulate_states(roots, model, 'sim', n_repetitions=3000)
    sim = np.stack([flat.nodes[i].sim for i in range(flat.n_nodes)])
    for n in zero:
        assert np.array_equal(sim[n], sim[flat.parent[n]])
    # with tau > 0 a zero branch has a positive length: some repetitions change state
    model = _model(kind, k, roots, tau=0.05)
    simulate_states(roots, model, 'sim', n_repetitions=3000)
    sim = np.stack([flat.nodes[i].sim for i in range(flat.n_nodes)])
    assert all(np.any(sim[n] != sim[flat.parent[n]]) for n in zero)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,k', [('F81', 7), ('F81', 300), ('JTT', 20)])
def test_reproducible_and_chunk_independent(kind, k, monkeypatch):
    roots, flat = _random_forest()
    model = _model(kind, k, roots, tau=0.1)
    k = len(model.states)
    np.random.seed(5)
    simulate_states(roots, model, 'a', n_repetitions=1000)
    a = np.stack([flat.nodes[i].a for i in range(flat.n_nodes)])
    np.random.seed(5)
    simulate_states(roots, model, 'b', n_repetitions=1000)
    b = np.stack([flat.nodes[i].b for i in range(flat.n_nodes)])
    assert np.array_equal(a, b)
    # a device budget that forces at least 3 chunks gives the same array
    es = 1 if k <= 256 else 2
    monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(2 * flat.n_nodes * es * 300))
    np.random.seed(5)
    simulate_states(roots, model, 'c', n_repetitions=1000)
    c = np.stack([flat.nodes[i].c for i in range(flat.n_nodes)])
    assert np.array_equal(a, c)
    monkeypatch.delenv('PASTML_AMD_DEVICE_BYTES')
    # the engine: one call of 1000 = (300 from 0) + (700 from 300); an offset that is not a multiple of 4 as well
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([model])
        whole = eng.simulate_states(1000, 1234)
        parts = np.concatenate([eng.simulate_states(300, 1234), eng.simulate_states(700, 1234, rep_offset=300)], axis=1)
        odd = np.concatenate([eng.simulate_states(301, 1234), eng.simulate_states(699, 1234, rep_offset=301)], axis=1)
        assert not np.array_equal(whole, eng.simulate_states(1000, 1235))
    assert np.array_equal(whole, parts)
    assert np.array_equal(whole, odd)


@pytest.mark.gpu
def test_engine_refuses_bad_arguments():
    flat = FlatForest.balanced(3)
    with hip.Engine(flat, 1, 4) as eng:
        with pytest.raises(hip.HipError):
            eng.simulate_states(10, 1)   # no model
        eng.set_models([(dict(kind=hip.KIND_F81, pi=np.full(4, 0.25)), (1.0, 0.0, 1.0))])
        with pytest.raises(hip.HipError):
            eng.simulate_states(0, 1)
        with pytest.raises(hip.HipError):
            eng.simulate_states(10, 1, col=1)
        with pytest.raises(hip.HipError):
            eng.simulate_states(10, 1, rep_offset=-4)
        assert eng.simulate_states(10, 1).shape == (flat.n_nodes, 10)


@pytest.mark.gpu
def test_marginal_counts_against_conditioned_simulation():
    """The reference's MRANDJCTest on the device: marginal_counts (50 000 scenarios) against 15 000 000 forward simulations
    kept where all tips agree with the data, transitions counted with the diagonal correction (MRANDJCTest.py:37-58)."""
    tree = read_tree(os.path.join(DATA, 'Albanian.minitree.tre'))
    character = 'Country'
    df = pd.read_csv(os.path.join(DATA, 'data.txt'), index_col=0, header=0)[[character]]
    preannotate_forest([tree], df=df)
    states = np.sort(np.array([_ for _ in df[character].unique() if not pd.isna(_) and '' != _]))
    model = JCModel(forest_stats=ForestStats([tree]), states=states,
                    parameter_file=os.path.join(DATA, 'params.character_Country.method_MPPA.model_JC.tab'))
    np.random.seed(239)
    n_repetitions = 50_000
    counts = ml.marginal_counts([tree], character, model, n_repetitions=n_repetitions)

    sim_character = character + '.simulated'
    n_sim = n_repetitions * 300
    simulate_states(tree, model, character=sim_character, n_repetitions=n_sim)
    k = len(states)
    state2id = dict(zip(states, range(k)))
    good = np.ones(n_sim, dtype=bool)
    for tip in tree:
        good &= getattr(tip, sim_character) == state2id[next(iter(getattr(tip, character)))]
    n_good = int(np.count_nonzero(good))
    assert n_good > 10_000
    sim_counts = np.zeros((k, k), dtype=np.float64)
    for n in tree.traverse('levelorder'):
        if n.is_leaf():
            continue
        frm = getattr(n, sim_character)[good].astype(np.int64)
        same = np.zeros(k)
        for c in n.children:
            to = getattr(c, sim_character)[good].astype(np.int64)
            t = np.zeros((k, k))
            np.add.at(t, (frm, to), 1)
            sim_counts += t
            same += np.diag(t)
        sim_counts[np.arange(k), np.arange(k)] -= np.minimum(np.bincount(frm, minlength=k), same)
    sim_counts /= n_good
    for i in range(k):
        for j in range(k):
            assert round(abs(counts[i, j] - sim_counts[i, j]), 2) == 0, (states[i], states[j], counts[i, j], sim_counts[i, j])


def _two_sample_p(a, b):
    """Two-sample chi-square (2 x k contingency, columns of small expectation pooled) p-value; None if nothing to test."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    tot = a + b
    exp_a = tot * a.sum() / tot.sum()
    exp_b = tot * b.sum() / tot.sum()
    big = np.minimum(exp_a, exp_b) >= 5
    cols_a, cols_b = list(a[big]), list(b[big])
    if (~big).any() and tot[~big].sum() > 0:
        cols_a.append(a[~big].sum())
        cols_b.append(b[~big].sum())
    if len(cols_a) < 2:
        return None
    table = np.array([cols_a, cols_b])
    if (table.sum(axis=0) == 0).any():
        return None
    return float(stats.chi2_contingency(table, correction=False)[1])


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['f81', 'jtt'])
def test_statistical_parity_with_the_reference_simulator(which):
    """Per-node state histograms of 20 000 device simulations against the reference's (make_golden_simulate.py)."""
    z = load_golden('simulate_albania')
    tree = read_tree(os.path.join(DATA, 'Albanian.tree.152tax.tre'))
    fs = ForestStats([tree])
    if which == 'f81':
        model = F81Model(states=z['f81_states'], forest_stats=fs, sf=float(z['f81_sf']), frequencies=z['f81_frequencies'])
    else:
        model = JTTModel(forest_stats=fs, sf=float(z['jtt_sf']))
    n_rep = int(z['n_repetitions'])
    np.random.seed(17)
    simulate_states(tree, model, 'sim', n_repetitions=n_rep)
    nodes = list(tree.traverse('levelorder'))
    assert [n.name for n in nodes] == [str(x) for x in z['names']]
    k = len(model.states)
    ref = z[which + '_hist']
    pvals = []
    trans = np.zeros((k, k), dtype=np.int64)
    for i, n in enumerate(nodes):
        ours = np.bincount(n.sim, minlength=k)
        q = _two_sample_p(ours, ref[i])
        if q is not None:
            pvals.append(q)
        if not n.is_root():
            np.add.at(trans, (n.up.sim.astype(np.int64), n.sim.astype(np.int64)), 1)
    assert min(pvals) > ALPHA / len(pvals), 'min p = {:.3g} over {} tests'.format(min(pvals), len(pvals))
    # the summed (parent, child) table: its pairs share the repetition (a root's state reaches every branch), so only the
    # repetitions are independent.  A cell's share of one repetition's branches lies in [0, 1]: sd <= 0.5, so the mean over
    # n_rep repetitions of each sample has sd <= 0.5 / sqrt(n_rep) (0.0035), the difference of two <= 0.005; 5 sd: 0.025
    n_branches = len(nodes) - 1
    diff = np.abs(trans - z[which + '_trans']) / float(n_rep * n_branches)
    assert diff.max() < 5 * np.sqrt(2) * 0.5 / np.sqrt(n_rep), diff.max()


@pytest.mark.gpu
def test_closed_loop_through_acr():
    """Simulate 8 columns of F81 (k = 4) on 65 536 tips, hand the tips to one acr() call, recover pi and sf.

    Tolerances (not tuned to a run).  Tip counts are no basis: on this tree neighbouring tips share most of their history.
    What informs the ML estimates are the substitutions: under F81 every event draws its new state from pi, at a rate
    mu = 1 / (1 - sum pi^2) = 1.74 per unit of sf * t, so the 131 070 branches (mean length 0.105) carry ~24 000 events,
    a multinomial sample of pi.  The events are not observed but inferred from the tips; allowing for that with a quarter
    of them (6 000), a frequency has sd <= sqrt(0.25 / 6000) = 0.0065, and 0.03 is 4.6 sd (32 frequencies checked).  The
    scaling factor sets the expected number of events: relative sd ~ 1 / sqrt(6000) = 1.3 %, and 10 % is 7.7 sd."""
    flat = FlatForest.balanced(16)
    roots, flat = _forest(flat)
    k = 4
    pi = np.array([0.6, 0.15, 0.2, 0.05])
    states = np.array(['A', 'B', 'C', 'D'])
    sf = 1.0
    model = F81Model(states=states, forest_stats=ForestStats(roots), sf=sf, frequencies=pi)
    np.random.seed(2024)
    n_cols = 8
    simulate_states(roots, model, 'sim', n_repetitions=n_cols)
    tips = flat.tips
    sim = np.stack([flat.nodes[i].sim for i in tips])
    df = pd.DataFrame({'c{}'.format(j): states[sim[:, j]] for j in range(n_cols)},
                      index=[flat.nodes[i].name for i in tips])
    res = acr(roots, df=df, prediction_method=MPPA, model=F81)
    assert len(res) == n_cols
    for r in res:
        m = r[MODEL]
        assert list(m.states) == list(states)
        np.testing.assert_allclose(m.frequencies, pi, atol=0.03)
        assert abs(m.sf / sf - 1) < 0.10, m.sf


@pytest.mark.gpu
def test_custom_rates_with_jtt_matrix_equals_jtt_on_simulated_data(tmp_path):
    """The reference's CUSTOM_RATESTest: simulate JTT data, then acr() under JTT and under CUSTOM_RATES with JTT's matrix and
    the JTT run's parameters give the same log-likelihood and marginal probabilities."""
    tree = read_tree(os.path.join(DATA, 'Albanian.tree.152tax.tre'))
    model = JTTModel(forest_stats=ForestStats([tree]), sf=2.0)
    np.random.seed(44)
    simulate_states(tree, model, 'sim', n_repetitions=1)
    for tip in tree:
        s = {JTT_STATES[int(tip.sim[0])]}
        tip.add_feature('state1', s)
        tip.add_feature('state2', set(s))
    r_jtt = acr(tree, columns=['state1'], column2states={'state1': JTT_STATES}, prediction_method=MPPA, model=JTT)[0]
    params = str(tmp_path / 'params.tab')
    with open(params, 'w') as f:
        f.write('parameter\tvalue\n')
        r_jtt[MODEL].save_parameters(f)
    rm = str(tmp_path / 'rate_matrix.txt')
    save_matrix(JTT_STATES, JTT_RATE_MATRIX, rm)
    r_cr = acr(tree, columns=['state2'], prediction_method=MPPA, model=CUSTOM_RATES,
               column2parameters={'state2': params}, column2rates={'state2': rm},
               column2states={'state2': JTT_STATES})[0]
    assert r_jtt[LOG_LIKELIHOOD] == r_cr[LOG_LIKELIHOOD]
    assert np.all(r_jtt[MARGINAL_PROBABILITIES].values == r_cr[MARGINAL_PROBABILITIES].values)
