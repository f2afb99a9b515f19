"""The restatement of the scenario sampler (tests/scenario_ref.py) is the right law: on a tree small enough to enumerate,
the root posterior times the restated conditionals is the exact joint posterior of the oracle's P(t); the restated draws follow
it; scenario_transition_counts against a loop.  No GPU."""
import itertools

import numpy as np

import scenario_ref as ref
from oracle import pastml_oracle as orc
from pastml_amd.tree import FlatForest
from pastml_amd.utilities.scenario_sampler import scenario_transition_counts

K = 3


def _tree():
    """5 tips, a polytomy at the root: 0 -> (1, 2, 3), 1 -> (4, 5), 3 -> (6, 7); 2, 4, 5, 6, 7 are tips."""
    parent = np.array([-1, 0, 0, 0, 1, 1, 3, 3], dtype=np.int32)
    n_children = np.array([3, 2, 0, 2, 0, 0, 0, 0], dtype=np.int32)
    first_child = np.array([1, 4, 0, 6, 0, 0, 0, 0], dtype=np.int32)
    dist = np.array([0.0, 0.21, 0.4, 0.08, 0.15, 0.3, 0.05, 0.6])
    return FlatForest(parent, n_children, first_child, dist, np.array([0]))


def _masks(flat):
    """Tips observed, one ambiguous (two states)."""
    m = np.ones((flat.n_nodes, K), dtype=int)
    for t, allowed in zip((2, 4, 5, 6, 7), ((0,), (1,), (0, 2), (2,), (1,))):
        m[t] = 0
        m[t, list(allowed)] = 1
    return m


def _specs():
    rng = np.random.default_rng(11)
    pi = rng.dirichlet(np.ones(K) * 3)
    yield 'F81', dict(kind=orc.KIND_F81, pi=pi), 1.4
    rates = np.triu(rng.uniform(0.2, 3, size=(K, K)), 1)
    d, a, ainv = orc.diagonalise(pi, rates + rates.T)
    yield 'CUSTOM_RATES', dict(kind=orc.KIND_EIGEN, pi=pi, d=d, A=a, Ainv=ainv), 0.9


def _inputs(flat, spec, sf):
    P = np.stack([orc.pij(spec, float(t), sf) for t in flat.dist])
    if spec['kind'] == orc.KIND_F81:
        return P, dict(E=P[:, 0, 0] - P[:, 1, 0])   # P_aa - P_ba = e
    return P, dict(P=P)


def _exact_joint(flat, masks, pi, P):
    """Every assignment of the 8 nodes with its posterior probability, by brute force."""
    assignments = np.array(list(itertools.product(range(K), repeat=flat.n_nodes)))
    prob = pi[assignments[:, 0]] * masks[0][assignments[:, 0]]
    for n in range(1, flat.n_nodes):
        prob = prob * P[n][assignments[:, flat.parent[n]], assignments[:, n]] * masks[n][assignments[:, n]]
    return assignments, prob / prob.sum()


def test_restated_conditionals_are_the_joint_posterior():
    flat = _tree()
    masks = _masks(flat)
    for name, spec, sf in _specs():
        P, inputs = _inputs(flat, spec, sf)
        r = orc.full_marginal_pass(flat, masks, spec, sf=sf)
        cond = ref.conditional_probabilities(flat, masks, r['bu'], spec['pi'], **inputs)
        assignments, exact = _exact_joint(flat, masks, spec['pi'], P)
        ours = r['posterior'][0][assignments[:, 0]]
        for n in range(1, flat.n_nodes):
            c = cond[n][assignments[:, flat.parent[n]], assignments[:, n]]
            ours = ours * np.where(ours > 0, c, 0.0)   # (rows of impossible parent states are never used)
        live = exact > 0
        assert live.sum() > 20, name
        assert np.all(ours[~live] == 0), name
        rel = np.abs(ours[live] - exact[live]) / exact[live]
        assert rel.max() <= 1e-12, '{}: {}'.format(name, rel.max())


def test_restated_draws_follow_the_joint_posterior():
    """Frequencies of whole scenarios against the exact joint (pooled chi-square at sampler_ref's ALPHA); conditioning on
    the restated parents reproduces the run; chunks of repetitions make up the whole; no fallback, no state outside a mask."""
    flat = _tree()
    masks = _masks(flat)
    n_rep = 20000
    for i, (name, spec, sf) in enumerate(_specs()):
        P, inputs = _inputs(flat, spec, sf)
        r = orc.full_marginal_pass(flat, masks, spec, sf=sf)
        args = (flat, masks, r['bu'], r['posterior'], spec['pi'])
        seed = (3 << 32) + 17 + i
        out = ref.scenarios(*args, seed, n_rep, rep_offset=5, **inputs)
        s = out['states']
        assert out['n_fallback'] == 0
        assert np.all(masks[np.arange(flat.n_nodes)[:, None], s] == 1)
        assignments, exact = _exact_joint(flat, masks, spec['pi'], P)
        code = (s * K ** np.arange(flat.n_nodes - 1, -1, -1)[:, None]).sum(axis=0)
        p = ref._pooled_chi2(np.bincount(code, minlength=len(exact)), n_rep * exact)
        assert p is not None and p > ref.ALPHA, '{}: p = {}'.format(name, p)
        again = ref.scenarios(*args, seed, n_rep, rep_offset=5, parent_states=s, **inputs)
        assert np.array_equal(again['states'], s)
        parts = np.concatenate([ref.scenarios(*args, seed, 6, rep_offset=5, **inputs)['states'],
                                ref.scenarios(*args, seed, 124, rep_offset=11, **inputs)['states']], axis=1)
        assert np.array_equal(parts, s[:, :130])
        assert not np.array_equal(ref.scenarios(*args, seed + 1, 130, rep_offset=5, **inputs)['states'], s[:, :130])


def test_fallback_draws_from_the_posterior_row():
    """A (node, parent state) without weight draws from the node's posterior row with the same uniform, and is counted."""
    flat = _tree()
    masks = _masks(flat)
    _, spec, sf = next(_specs())
    P, inputs = _inputs(flat, spec, sf)
    r = orc.full_marginal_pass(flat, masks, spec, sf=sf)
    bu = r['bu'].copy()
    bu[3] = 0.0   # node 3 loses every weight
    n_rep = 500
    forced = np.zeros((flat.n_nodes, n_rep), dtype=np.int64)
    out = ref.scenarios(flat, masks, bu, r['posterior'], spec['pi'], 9, n_rep, parent_states=forced, **inputs)
    assert out['n_fallback'] == n_rep
    u = ref.scen_uniforms(9, 3, np.arange(n_rep))
    cum = np.cumsum(r['posterior'][3])
    want = np.array([int(np.argmax(cum > x * cum[-1])) for x in u])
    assert np.array_equal(out['states'][3], want)


def test_scenario_transition_counts_against_a_loop():
    flat = FlatForest.random(30, seed=4, max_arity=4, n_trees=2)
    roots = flat.to_tree_nodes()
    rng = np.random.default_rng(1)
    k, n_rep = 5, 17
    states = rng.integers(0, k, size=(flat.n_nodes, n_rep)).astype(np.uint8)
    from pastml_amd.tree import ArrayColumn
    flat.set_column('c', ArrayColumn(states))
    got = scenario_transition_counts(roots, 'c', k)
    assert got.shape == (n_rep, k, k)
    assert np.array_equal(got, ref.transition_counts_loop(flat, states, k))
    assert np.all(got.sum(axis=(1, 2)) == flat.n_nodes - len(flat.roots))
