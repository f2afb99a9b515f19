"""
CPU-only: the law of the history sampler per time interval (tests/history_time_sample_ref.py, the restatement the device is held
to draw for draw), with no device.  With one bin that covers the tree it has to reproduce history_sample_ref.histories; cut into
bins, the bins have to sum to the same, no event may be counted twice or lost, the lineages have to be the branches that cross
each boundary, and the means have to be the closed forms of history_time_ref.by_coefficients (60 digits) within 5 standard errors.
"""
import math
from types import SimpleNamespace

import numpy as np

import expected_history_ref as href
import history_time_ref as ht
import history_time_sample_ref as hts
import scenario_ref
from loglik_gradient_ref import _vectors
from pastml_amd.tree import FlatForest

SEED = (13 << 32) + 4711
K = 3
PI = np.array([0.55, 0.3, 0.15])
TAU = 0.05
BOUND = 5.0   # standard errors: a condition of the law, not a knob


def _inputs(n_tips, seed, n_trees=1, x_top=3.0):
    flat = FlatForest.random(n_tips, seed=seed, max_arity=3, n_trees=n_trees)
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[::3]] *= 20.0
    mu = 1.0 / (1.0 - PI.dot(PI))
    sf = x_top / (mu * (flat.dist[branches] + TAU).max())
    rng = np.random.default_rng(seed + 100)
    masks = np.ones((flat.n_nodes, K), dtype=np.int8)
    for t in flat.tips:
        if rng.random() < 0.1:
            continue                             # missing
        masks[t] = 0
        masks[t, rng.choice(K, p=PI)] = 1
    return flat, masks, sf


def _scenarios(flat, masks, sf, n_rep):
    _, _, e, v, _, q, _ = _vectors(flat, masks, [href._D(p) for p in PI], href._D(sf), href._D(TAU), href._D(1.0))
    E = np.array([float(z) for z in e])
    bu = np.array([[float(z) for z in row] for row in v])
    post = np.array([[float(z) for z in row] for row in q])
    scen = scenario_ref.scenarios(flat, masks, bu, post, PI, SEED, n_rep, E=E)
    assert scen['n_fallback'] == 0
    return scen['states'], E


_CACHE = {}


def _shared():
    """A forest of two trees with staggered roots, 256 repetitions; one covering bin and five with a boundary on a node."""
    if 'r' not in _CACHE:
        flat, masks, sf = _inputs(30, 5, n_trees=2)
        states, E = _scenarios(flat, masks, sf, 256)
        t = ht.root_distance(flat, stagger=0.37)
        one = hts.histories(flat, states, PI, E, sf, TAU, 1.0, SEED, t, ht.covering_boundaries(t, 1))
        T5 = ht.covering_boundaries(t, 5, on_node=True)
        five = hts.histories(flat, states, PI, E, sf, TAU, 1.0, SEED, t, T5)
        _CACHE['r'] = flat, t, T5, one, five
    return _CACHE['r']


def _within(got, r, slack=0.0):
    return (np.abs(got - r['times']) <= hts.bound(r) + slack).all()


def test_one_covering_bin_is_the_whole_tree_sampler():
    flat, t, _, one, _ = _shared()
    whole = one['whole']
    assert whole['events'].max() >= 3, 'no branch with several events'
    assert np.array_equal(one['jumps'][:, 0], whole['jumps'])
    assert np.array_equal(one['summands'][:, 0], whole['summands'])
    # the parent's dwell is (L w_i) / Wsum, this one L (c_{i+1} - c_i) where the branch has events: within this law's own bound
    assert _within(whole['times'][:, None, :], one)
    assert np.array_equal(one['events'], whole['events'])
    assert one['near'] == whole['near'] and len(one['near']) <= 2   # (no segment end strictly inside a branch)
    # lineages: nothing is alive at T_0, before the first root, and at T_1, after the last tip
    assert (one['lineages'] == 0).all()


def test_bins_sum_to_the_whole_and_lineages_are_the_crossing_branches():
    flat, t, T5, one, five = _shared()
    whole = five['whole']
    assert np.array_equal(five['jumps'].sum(axis=1), whole['jumps'])
    total = dict(times=five['times'].sum(axis=1), summands=five['summands'].sum(axis=1), scale=five['scale'].sum(axis=1))
    assert (np.abs(whole['times'] - total['times']) <= hts.bound(total)).all()
    assert (five['scale'] > 0).any() and (five['summands'].sum(axis=1) >= whole['summands']).all()
    crossing = ht.crossing(flat.parent, t, T5)
    assert crossing[1:-1].min() > 0
    assert np.array_equal(five['lineages'].sum(axis=-1), np.broadcast_to(crossing, (256, 6)))
    # a boundary lies on a node: the branches that begin there show their parent's state, those that end there are not alive
    sp = five['plan']
    on = sp['starts'] & (sp['s1'] == 0.0)
    assert on.any()
    length = ((flat.dist[flat.parent >= 0] + TAU) * 1.0).sum()
    assert np.allclose(five['times'].sum(axis=(1, 2)), length, rtol=1e-12, atol=0)
    assert len(five['near']) <= 2, five['near']


def test_an_event_is_never_counted_twice():
    """One long branch cut into 50 bins: the jumps of the bins are the branch's, the dwells make up its length."""
    n_rep, x = 512, 30.0
    mu = 1.0 / (1.0 - PI.dot(PI))
    flat = SimpleNamespace(parent=np.array([-1, 0]), dist=np.array([0.0, x / mu]))
    states = np.empty((2, n_rep), dtype=np.int64)
    states[0], states[1] = 0, 1
    E = np.array([1.0, math.exp(-x)])
    t = np.array([0.25, 0.25 + x / mu])
    T = np.linspace(t[0], t[1], 51)
    T[0] -= 0.1
    T[-1] += 0.1
    r = hts.histories(flat, states, PI, E, 1.0, 0.0, 1.0, SEED, t, T)
    whole = r['whole']
    assert whole['events'][1].min() >= 1 and whole['events'][1].mean() > 20
    assert np.array_equal(r['jumps'].sum(axis=1), whole['jumps'])
    assert np.array_equal(r['jumps'].sum(axis=(1, 2, 3)), whole['branch_jumps'][1])
    assert np.allclose(r['times'].sum(axis=(1, 2)), x / mu, rtol=1e-13, atol=0)
    sp = r['plan']
    own = sp['node'] == 1
    assert own.sum() == 50 and np.array_equal(sp['s2'][own][:-1], sp['s1'][own][1:]) and sp['ends'][own][-1]
    assert (r['lineages'].sum(axis=-1)[:, 1:50] == 1).all() and (r['lineages'][:, [0, 50]] == 0).all()
    # the lineage at a boundary is the state the dwell just behind it is spent in: it ends in 1, the child's state
    assert (r['lineages'][:, 1].argmax(axis=-1) == 0).mean() > 0.3   # (begins in 0)


def test_means_are_the_closed_forms_per_interval():
    n_rep = 4096
    flat, masks, sf = _inputs(9, 11, x_top=3.0)
    states, E = _scenarios(flat, masks, sf, n_rep)
    t = ht.root_distance(flat)
    T = ht.covering_boundaries(t, 3, on_node=True)
    r = hts.histories(flat, states, PI, E, sf, TAU, 1.0, SEED, t, T)
    exact = ht.by_coefficients(flat, masks, PI, t, T, sf, TAU, 1.0)
    checked = dict(times=0, jumps=0, lineages=0)

    def hold(kind, label, column, want):
        column = column.astype(np.float64)
        se = column.std(ddof=1) / math.sqrt(n_rep)
        z = abs(column.mean() - want) / se
        print('{}{}: mean {:.6g} exact {:.6g} z {:.2f}'.format(kind, label, column.mean(), want, z))
        assert z <= BOUND, (kind, label, z)
        checked[kind] += 1

    # a mean over 4096 repetitions is normal where the entry is hit often: every times entry of a bin the tree crosses; the
    # counts that expect a quarter of an event per repetition (a thousand events in all) or more
    for m in range(3):
        for s in range(K):
            hold('times', (m, s), r['times'][:, m, s], float(exact['times'][m][s]))
            for j in range(K):
                if j != s and float(exact['jumps'][m][s][j]) >= 0.25:
                    hold('jumps', (m, s, j), r['jumps'][:, m, s, j], float(exact['jumps'][m][s][j]))
    for m in range(4):
        for s in range(K):
            if float(exact['lineages'][m][s]) >= 0.25:
                hold('lineages', (m, s), r['lineages'][:, m, s], float(exact['lineages'][m][s]))
    assert checked['times'] == 9 and checked['jumps'] >= 4 and checked['lineages'] >= 4, checked
