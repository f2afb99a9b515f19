"""
The numpy restatement of the exact expected transition counts (tests/expected_counts_ref.py) against the reference's own
marginal_counts estimates (tests/golden/marginal_counts.npz, 40 000 repetitions: JC on 64 tips, and Albania / F81 at the
optimum, whose zero-length tips bring the altered rules in), plus the identities of the definition and the argument
handling of pastml_amd.utilities.transition_counter.  No GPU.
"""
import os

import numpy as np
import pandas as pd
import pytest

import expected_counts_ref as xref
from conftest import load_golden, GOLDEN
from oracle import pastml_oracle as orc
from pastml_amd import ml, synthetic
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.models.F81Model import F81Model, F81
from pastml_amd.models.JCModel import JC
from pastml_amd.tree import FlatForest, read_tree

DATA = os.path.join(GOLDEN, 'data')
TREE_NWK = os.path.join(DATA, 'Albanian.tree.152tax.tre')
STATES_INPUT = os.path.join(DATA, 'data.txt')
PARAMS_JC = os.path.join(DATA, 'params.character_Country.method_MPPA.model_JC.tab')


def bound(ref, n_rep, extra):
    """tests/test_gpu_api.py::test_marginal_counts_statistical_parity's bound for two independent estimates"""
    return 6 * np.sqrt(np.maximum(ref, 0.05) / n_rep) * 3 + extra


def albania_case():
    """(flat, masks as the marginal pass sees them, altered, initial masks, spec, sf) of Albania / F81 at the optimum"""
    zz = load_golden('albania_F81')
    tree = read_tree(TREE_NWK)
    preannotate_forest([tree], df=pd.read_csv(STATES_INPUT, index_col=0, header=0)[['Country']])
    model = F81Model(states=zz['opt_states'], forest_stats=ForestStats([tree]), sf=float(zz['opt_sf']),
                     frequencies=zz['opt_frequencies'])
    model.freeze()
    problem = ml.ForestProblem([tree], 'Country', model.states)
    problem.initialize_allowed_states()
    altered_ids = problem.alter_zero_node_allowed_states()
    altered = np.zeros(problem.N, dtype=bool)
    altered[altered_ids] = True
    spec = dict(kind=orc.KIND_F81, pi=np.asarray(model.frequencies, dtype=np.float64))
    return problem.flat, problem.masks.astype(int), altered, problem.init_masks.astype(int), spec, float(model.sf), tree, model


def test_restatement_agrees_with_the_reference_jc():
    z = load_golden('marginal_counts')
    n_rep = int(z['n_repetitions'])
    flat = synthetic.balanced_forest(6)
    k = 4
    masks = np.ones((flat.n_nodes, k), dtype=int)
    masks[flat.tips] = 0
    masks[flat.tips, z['jc_tip_states']] = 1
    spec = dict(kind=orc.KIND_F81, pi=np.full(k, 0.25))
    out = xref.from_oracle(orc, flat, masks, spec, sf=float(z['jc_sf']))
    want = z['jc_counts']
    diff = np.abs(out['counts'] - want)
    print('JC: max |exact - reference estimate| =', diff.max(), 'entries', want.min(), '..', want.max())
    assert np.all(diff < bound(want, n_rep, 0.02)), diff.max()
    # the propagated state frequencies are the marginal posteriors (reversible model)
    np.testing.assert_allclose(out['q'], out['posterior'], rtol=0, atol=1e-12)


def test_restatement_agrees_with_the_reference_albania_altered():
    z = load_golden('marginal_counts')
    n_rep = int(z['n_repetitions'])
    flat, masks, altered, initial, spec, sf, _, _ = albania_case()
    assert altered.any()
    out = xref.from_oracle(orc, flat, masks, spec, sf=sf, altered=altered, initial=initial)
    want = z['albania_counts']
    diff = np.abs(out['counts'] - want)
    print('Albania: max |exact - reference estimate| =', diff.max(), 'altered nodes', int(altered.sum()))
    assert np.all(diff < bound(want, n_rep, 0.03)), (diff.max(), out['counts'].round(3), want.round(3))
    np.testing.assert_allclose(out['q'], out['posterior'], rtol=0, atol=1e-12)


def test_host_assembly_of_altered_pairs_is_the_restatement():
    """ml.add_altered_pairs (vectorised over the affected parents) on the restatement's own unaltered part."""
    flat, masks, altered, initial, spec, sf, _, _ = albania_case()
    full = xref.from_oracle(orc, flat, masks, spec, sf=sf, altered=altered, initial=initial)
    # the device's share: pairs without an altered end, diagonal corrected for the parents without such a pair
    k = masks.shape[1]
    r = orc.full_marginal_pass(flat, masks, spec, sf=sf)
    post = r['posterior']
    counts = np.zeros((k, k))
    same = np.zeros((flat.n_nodes, k))
    for p in np.flatnonzero(flat.n_children > 0):
        s = np.zeros(k)
        dirty = altered[p]
        for n in range(flat.first_child[p], flat.first_child[p] + flat.n_children[p]):
            if altered[p] or altered[n]:
                dirty = True
                continue
            w = r['bu'][n] * spec['pi'] * masks[n]
            weights = w[None, :] * orc.pij(spec, float(flat.dist[n]), sf).T
            den = weights.sum(axis=1)
            ok = (post[p] > 0) & (den > 0)
            M = np.zeros((k, k))
            M[ok] = weights[ok] / den[ok, None]
            counts += post[p][:, None] * M
            s += post[p] * M.diagonal()
        if dirty:
            same[p] = s
        else:
            counts[np.arange(k), np.arange(k)] -= np.minimum(post[p], s)
    got = ml.add_altered_pairs(flat, counts, same, post, altered, initial)
    np.testing.assert_allclose(got, full['counts'], rtol=1e-12, atol=1e-12)
    # nothing altered: the device's sums come back as they are
    none = np.zeros(flat.n_nodes, dtype=bool)
    assert np.array_equal(ml.add_altered_pairs(flat, counts, same, post, none, initial), counts)


def test_two_tip_tree_by_hand():
    """Root with tips A (state 0) and B (state 1), JC with two states, e = exp(-2 t) per branch (mu = 2).
    Root posterior q ~ (P00(ta) P10(tb), P01(ta) P11(tb)) pi; a tip's conditional puts everything on its state, so
    result[a][s_tip] += q[a]; same[a] = q[a] for both a (each state has one tip that stays), the correction takes
    min(q[a], q[a]) = q[a] off the diagonal: counts = [[0, q0], [q1, 0]]."""
    flat = FlatForest.from_trees([read_tree('(A:0.3,B:0.7);')])
    k = 2
    masks = np.ones((3, k), dtype=int)
    tips = list(flat.tips)
    masks[tips[0]] = [1, 0]
    masks[tips[1]] = [0, 1]
    spec = dict(kind=orc.KIND_F81, pi=np.full(k, 0.5))
    out = xref.from_oracle(orc, flat, masks, spec)
    ea, eb = np.exp(-2 * flat.dist[tips[0]]), np.exp(-2 * flat.dist[tips[1]])
    same_a, diff_a = 0.5 * (1 + ea), 0.5 * (1 - ea)
    same_b, diff_b = 0.5 * (1 + eb), 0.5 * (1 - eb)
    q = np.array([same_a * diff_b, diff_a * same_b])
    q /= q.sum()
    np.testing.assert_allclose(out['counts'], [[0.0, q[0]], [q[1], 0.0]], rtol=0, atol=1e-15)


@pytest.mark.parametrize('k, seed', [(3, 1), (7, 2)])
def test_rows_of_the_uncorrected_counts_sum_to_the_parents_mass(k, seed):
    """sum_b of the uncorrected row a = sum over the branches of q_parent[a] (every M_n row sums to one)."""
    flat = FlatForest.random(60, seed=seed, max_arity=4, zero_frac=0.0, n_trees=2)
    rng = np.random.default_rng(seed)
    masks = np.ones((flat.n_nodes, k), dtype=int)
    states = rng.integers(0, k, size=len(flat.tips))
    masks[flat.tips] = 0
    masks[flat.tips, states] = 1
    masks[flat.tips[::7]] = 1   # missing tips
    spec = dict(kind=orc.KIND_F81, pi=rng.dirichlet(np.ones(k) * 3))
    out = xref.from_oracle(orc, flat, masks, spec, sf=1.3, tau=0.05, tf=0.9)
    np.testing.assert_allclose(out['uncorrected'].sum(axis=1), out['branch_mass'], rtol=1e-12)
    np.testing.assert_allclose(out['q'], out['posterior'], rtol=0, atol=1e-12)
    assert np.all(out['counts'] > -1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# count_transitions: argument handling, with the device part mocked
# ---------------------------------------------------------------------------------------------------------------------

def test_count_transitions_argument_handling(tmp_path, monkeypatch):
    from pastml_amd.utilities import transition_counter as tc
    calls = []

    def fake_expected(forest, characters, models):
        calls.append(('expected', list(characters), [type(m).__name__ for m in models]))
        return [np.full((len(m.states), len(m.states)), 1.0 + i) for i, m in enumerate(models)]

    def fake_sampled(forest, character, model, n_repetitions=1000):
        calls.append(('sampled', character, n_repetitions))
        return np.zeros((len(model.states), len(model.states)))

    monkeypatch.setattr(tc, 'expected_counts', fake_expected)
    monkeypatch.setattr(tc, 'marginal_counts', fake_sampled)
    out = str(tmp_path / 'counts.tab')
    tc.count_transitions(TREE_NWK, STATES_INPUT, 'Country', PARAMS_JC, out, data_sep=',', model=JC, n_repetitions=None)
    assert calls == [('expected', ['Country'], ['JCModel'])]
    table = pd.read_csv(out, sep='\t', index_col=0)
    assert table.index.name == 'from'
    assert list(table.columns) == list(table.index) == ['Africa', 'Albania', 'EastEurope', 'Greece', 'WestEurope']
    assert np.all(table.values == 1.0)
    # the sampler when repetitions are asked for
    tc.count_transitions(TREE_NWK, STATES_INPUT, 'Country', PARAMS_JC, out, data_sep=',', model=JC, n_repetitions=25)
    assert calls[-1] == ('sampled', 'Country', 25)
    # several columns: a template, one call
    del calls[:]
    df = pd.read_csv(STATES_INPUT, index_col=0, header=0)
    df['Region'] = df['Country']
    two = str(tmp_path / 'two.csv')
    df.to_csv(two)
    template = str(tmp_path / 'counts.{column}.tab')
    tc.count_transitions(TREE_NWK, two, ['Country', 'Region'], [PARAMS_JC, PARAMS_JC], template, data_sep=',',
                         model=JC, n_repetitions=0)
    assert len(calls) == 1 and calls[0][1] == ['Country', 'Region']
    assert pd.read_csv(str(tmp_path / 'counts.Country.tab'), sep='\t', index_col=0).values[0, 0] == 1.0
    assert pd.read_csv(str(tmp_path / 'counts.Region.tab'), sep='\t', index_col=0).values[0, 0] == 2.0
    with pytest.raises(ValueError):
        tc.count_transitions(TREE_NWK, two, ['Country', 'Region'], [PARAMS_JC, PARAMS_JC], out, data_sep=',', model=JC,
                             n_repetitions=None)
    with pytest.raises(NotImplementedError):
        tc.count_transitions(TREE_NWK, STATES_INPUT, 'Country', PARAMS_JC, out, data_sep=',', model=JC, html='x.html')
