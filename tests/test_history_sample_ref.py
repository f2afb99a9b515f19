"""
CPU-only: the law of the history sampler itself (tests/history_sample_ref.py, the restatement the device is held to draw for
draw), with no device.  On a small forest the restated histories have to satisfy, per repetition, the identities a history
satisfies, and their means have to be the closed form of expected_history_ref.history (60 digits) within 5 standard errors; on a
single branch the number of events has to follow the zero-truncated Poisson law, with the mass at zero when the ends agree.
"""
import math
from types import SimpleNamespace

import numpy as np

import expected_history_ref as href
import history_sample_ref as hs
import scenario_ref
from loglik_gradient_ref import _vectors
from sampler_ref import _pooled_chi2, ALPHA
from pastml_amd.tree import FlatForest

R = 4096
SEED = (11 << 32) + 20240
K = 3
PI = np.array([0.55, 0.3, 0.15])
TAU = 0.05
BOUND = 5.0   # standard errors: a condition of the law, not a knob


def _inputs():
    flat = FlatForest.random(40, seed=3, max_arity=3)
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[::3]] *= 50.0             # (tau bounds d_n + tau below: long branches for a range of 300)
    mu = 1.0 / (1.0 - PI.dot(PI))
    d = flat.dist[branches] + TAU
    sf = 3.0 / (mu * d.max())                    # x_n = mu (d_n + tau) sf: 3 on the longest branch, about 0.01 on the shortest
    x = mu * d * sf
    assert x.min() < 0.02 and x.max() > 2.9, (x.min(), x.max())
    rng = np.random.default_rng(17)
    masks = np.ones((flat.n_nodes, K), dtype=np.int8)
    for t in flat.tips:
        u = rng.random()
        if u < 0.1:
            continue                             # missing
        masks[t] = 0
        if u < 0.25:
            masks[t, rng.choice(K, size=2, replace=False)] = 1   # ambiguous
        else:
            masks[t, rng.choice(K, p=PI)] = 1
    return flat, masks, sf


def _restated():
    flat, masks, sf = _inputs()
    _, _, e, v, _, q, _ = _vectors(flat, masks, [href._D(p) for p in PI], href._D(sf), href._D(TAU), href._D(1.0))
    E = np.array([float(z) for z in e])
    bu = np.array([[float(z) for z in row] for row in v])
    post = np.array([[float(z) for z in row] for row in q])
    scen = scenario_ref.scenarios(flat, masks, bu, post, PI, SEED, R, E=E)
    assert scen['n_fallback'] == 0
    out = hs.histories(flat, scen['states'], PI, E, sf, TAU, 1.0, SEED)
    exact = href.history(flat, masks, PI, sf, TAU, 1.0)
    return flat, scen['states'], out, exact


_CACHE = {}


def _shared():
    if 'r' not in _CACHE:
        _CACHE['r'] = _restated()
    return _CACHE['r']


def test_small_x_range():
    flat, masks, sf = _inputs()
    _, x, _ = hs.branch_scalars(flat, PI, sf, TAU, 1.0)
    x = x[flat.parent >= 0]
    print('x_n from {:.3g} to {:.3g}'.format(x.min(), x.max()))
    assert 0.005 <= x.min() <= 0.02 and 2.9 <= x.max() <= 3.0 + 1e-9


def test_identities_per_repetition():
    flat, states, out, exact = _shared()
    branches = np.flatnonzero(flat.parent >= 0)
    length = float(exact['tree_length'])
    total = out['times'].sum(axis=1)
    n_sum = out['summands'].sum(axis=1)
    assert (np.abs(total - length) <= (n_sum + 16) * 2.0 ** -52 * length).all(), np.abs(total - length).max()
    jumps = out['jumps'].astype(np.int64)
    assert (jumps[:, np.arange(K), np.arange(K)] == 0).all()
    assert np.array_equal(jumps.sum(axis=(1, 2)), out['branch_jumps'].astype(np.int64).sum(axis=0))
    assert (out['branch_jumps'][flat.parent < 0] == 0).all()
    # I2 of expected_history_ref.identities, per draw: what flows into a state minus what flows out of it is the number of
    # children in it minus the number of parents in it
    child = np.stack([(states[branches] == i).sum(axis=0) for i in range(K)], axis=1)
    par = np.stack([(states[flat.parent[branches]] == i).sum(axis=0) for i in range(K)], axis=1)
    assert np.array_equal(jumps.sum(axis=1) - jumps.sum(axis=2), child - par)
    # a branch whose ends differ has at least one jump; the events bound the jumps
    differ = states[branches] != states[flat.parent[branches]]
    assert (out['branch_jumps'][branches][differ] >= 1).all()
    assert (out['branch_jumps'].astype(np.int64) <= out['events']).all()
    assert len(out['near']) <= 2, out['near']


def test_means_are_the_closed_form():
    _, _, out, exact = _shared()
    checked_times = checked_jumps = 0
    for s in range(K):
        col = out['times'][:, s]
        se = col.std(ddof=1) / math.sqrt(R)
        z = abs(col.mean() - float(exact['times'][s])) / se
        print('times[{}]: mean {:.6g} exact {:.6g} z {:.2f}'.format(s, col.mean(), float(exact['times'][s]), z))
        checked_times += 1
        assert z <= BOUND, (s, z)
    for i in range(K):
        for j in range(K):
            if i == j or float(exact['jumps'][i][j]) < 1.0:
                continue
            col = out['jumps'][:, i, j].astype(np.float64)
            se = col.std(ddof=1) / math.sqrt(R)
            z = abs(col.mean() - float(exact['jumps'][i][j])) / se
            print('jumps[{}][{}]: mean {:.6g} exact {:.6g} z {:.2f}'.format(i, j, col.mean(), float(exact['jumps'][i][j]), z))
            checked_jumps += 1
            assert z <= BOUND, (i, j, z)
    assert checked_times >= K and checked_jumps >= 2, (checked_times, checked_jumps)
    # the per-branch means as well, on the branches that expect a tenth of a jump or more
    bj = out['branch_jumps'].astype(np.float64)
    for n, want in enumerate(exact['branch_jumps']):
        if float(want) >= 0.1:
            se = bj[n].std(ddof=1) / math.sqrt(R)
            assert abs(bj[n].mean() - float(want)) <= BOUND * se, (n, bj[n].mean(), float(want), se)


def _one_branch(a, b, x, n_rep, seed):
    mu = 1.0 / (1.0 - PI.dot(PI))
    flat = SimpleNamespace(parent=np.array([-1, 0]), dist=np.array([0.0, x / mu]))
    states = np.empty((2, n_rep), dtype=np.int64)
    states[0], states[1] = a, b
    E = np.array([1.0, math.exp(-x)])
    out = hs.histories(flat, states, PI, E, 1.0, 0.0, 1.0, seed)
    _, xs, L = hs.branch_scalars(flat, PI, 1.0, 0.0, 1.0)
    return out, xs[1], L[1]


def _truncated_poisson(x, top):
    m = np.arange(top + 1)
    logp = -x + m * math.log(x) - np.array([math.lgamma(i + 1.0) for i in m])
    return np.exp(logp)   # e x^m / m!, m = 0 .. top (entry 0: e)


CASES = [(0, 1, 30.0), (1, 1, 30.0), (2, 2, 1.0), (0, 0, 0.3), (0, 2, 0.3)]


def test_one_branch_event_counts_follow_the_zero_truncated_poisson():
    n_rep = 20000
    pvals = []
    for c, (a, b, x) in enumerate(CASES):
        out, xb, L = _one_branch(a, b, x, n_rep, SEED + 7 * c)
        M = out['events'][1]
        top = int(max(M.max(), 4 * x + 20))
        terms = _truncated_poisson(xb, top)
        weight = terms.copy()
        if a == b:
            weight[1:] *= PI[a]          # M >= 1 ends on b with probability pi_b; M = 0 stays: the mass e at zero
        else:
            weight[0] = 0.0
            assert M.min() >= 1
        expected = n_rep * weight / weight.sum()
        p = _pooled_chi2(np.bincount(M, minlength=top + 1), expected)
        print('a={} b={} x={}: mean M {:.4g}, M = 0 in {} of {} (expected {:.4g}), p {:.3g}'
              .format(a, b, x, M.mean(), int((M == 0).sum()), n_rep, expected[0], p))
        assert p is not None
        pvals.append(p)
        # the dwells of a repetition make up the branch
        assert np.allclose(out['times'].sum(axis=1), L, rtol=1e-13, atol=0)
    assert min(pvals) > ALPHA / len(pvals), pvals
