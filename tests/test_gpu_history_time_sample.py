"""
Histories per time interval drawn on the device (pml_sample_histories_through_time, Engine.sample_histories_through_time) draw for
draw against their restatement (tests/history_time_sample_ref.py) conditioned on the device's own scenarios and on the
exponentials the device stored (BUF_BRANCH_EXP), on the forests of test_gpu_scenarios.py dated by their root distances (staggered
roots) and cut by history_time_ref.covering_boundaries.

jumps and lineages are compared exactly.  times entry by entry within a bound of two parts, added together
(history_time_sample_ref.bound): (summands + 16) * 2^-52 relative -- all terms are non-negative, a dwell is a few rounded
operations, and a sum of m positive terms is off by at most m roundings --, and for every cut piece L (min - max) of the entry
(4 M_n + 16) * 2^-52 * L_n absolute: the piece is a difference of two positions, each a quotient of sums of up to M_n + 1 logs
good to an ulp.  The worst ratio seen is in profiles/history_time_sampler.txt.  The policy for draws at a boundary is that of
test_gpu_history_sample.py: a repetition with a (node, repetition) pair the restatement lists as near is left out of the
comparison, at most 2 pairs per case.
"""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest

import history_sample_ref as hs
import history_time_ref as ht
import history_time_sample_ref as hts
from conftest import load_golden, GOLDEN
from pastml_amd import hip, ml
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.models.F81Model import F81Model
from pastml_amd.models.HKYModel import HKYModel
from pastml_amd.tree import annotate_dates, read_tree
from test_gpu_scenarios import _forest, _spec, _masks, _marginal_pass

pytestmark = pytest.mark.gpu

MAX_NEAR = 2
BOUND = 5.0   # standard errors

DATA = os.path.join(GOLDEN, 'data')
TREE_NWK = os.path.join(DATA, 'Albanian.tree.152tax.tre')
STATES_INPUT = os.path.join(DATA, 'data.txt')


def _model(kind, k, flat, tree, x_top=None):
    spec, (sf, tau, tf) = _spec(kind, k, flat, tau=0.0 if tree == 'zero64' else 0.1)
    if x_top is not None:   # sf such that the longest branch has x = x_top
        mu = 1.0 / (1.0 - float(np.dot(spec['pi'], spec['pi'])))
        sf = x_top / (mu * (flat.dist[flat.parent >= 0].max() + tau) * tf)
    return spec, (sf, tau, tf)


def _times(flat, tree, M, span='cover'):
    """Node times (the roots of a forest 0.05 apart) and M + 1 boundaries: 'cover' -- the whole range, for M >= 2 with a
    boundary on a node --, 'middle' -- the middle third of it only."""
    t = ht.root_distance(flat, stagger=0.05)
    if tree == 'single':
        return t, np.linspace(-1.0, 1.0, M + 1)
    T = ht.covering_boundaries(t, M, on_node=True)
    if span == 'middle':
        lo, hi = T[0] + (T[-1] - T[0]) / 3.0, T[0] + 2.0 * (T[-1] - T[0]) / 3.0
        T = np.linspace(lo, hi, M + 1)
    return t, T


def _draw(flat, model, k, masks, t, T, n_rep, seed, rep_offset=0, tune=None, **what):
    with hip.Engine(flat, 1, k, tune=tune) as eng:
        _marginal_pass(eng, [model], masks)
        out = eng.sample_histories_through_time(t, T, n_rep, seed, rep_offset=rep_offset, **what)
        E = eng.download(hip.BUF_BRANCH_EXP, 0)
    return out, E


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def _check(flat, out, E, model, seed, rep_offset, t, T, label, covering):
    states, times, jumps, lineages, fallen = out
    spec, (sf, tau, tf) = model
    N, n_rep = states.shape
    k, M = len(spec['pi']), len(T) - 1
    assert times.shape == (n_rep, M, k) and times.dtype == np.float64, label
    assert jumps.shape == (n_rep, M, k, k) and jumps.dtype == np.uint32, label
    assert lineages.shape == (n_rep, M + 1, k) and lineages.dtype == np.uint32, label
    assert fallen == 0, label
    r = hts.histories(flat, states, spec['pi'], E, sf, tau, tf, seed, t, T, rep_offset)
    assert r['n_skipped'] == 0, label
    assert len(r['near']) <= MAX_NEAR, '{}: the restatement lists {} near pairs: pick another seed'.format(label, len(r['near']))
    keep = np.ones(n_rep, dtype=bool)
    keep[[rep for _, rep in r['near']]] = False
    assert np.array_equal(jumps[keep], r['jumps'][keep]), '{}: {} jumps entries differ'.format(
        label, int((jumps[keep] != r['jumps'][keep]).sum()))
    assert np.array_equal(lineages[keep], r['lineages'][keep]), '{}: {} lineages entries differ'.format(
        label, int((lineages[keep] != r['lineages'][keep]).sum()))
    want, limit = r['times'][keep], hts.bound(r)[keep]
    got = times[keep]
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(limit > 0, err / limit, np.where(err == 0.0, 0.0, np.inf))
    worst = float(ratio.max()) if ratio.size else 0.0
    print('{}: {} near pairs; times: worst error / bound {:.3g}, {} cut pieces, most events on a branch {}'.format(
        label, len(r['near']), worst, int((r['scale'] > 0).sum()), int(r['events'].max()) if r['events'].size else 0))
    assert worst <= 1.0, (label, worst)
    # the identities of a history cut into bins, on the device's own output
    crossing = ht.crossing(flat.parent, t, T)
    assert np.array_equal(lineages.sum(axis=-1), np.broadcast_to(crossing, (n_rep, M + 1))), label
    assert (jumps[:, :, np.arange(k), np.arange(k)] == 0).all(), label
    if covering:
        length = ((flat.dist[flat.parent >= 0] + tau) * tf).sum()
        assert np.allclose(times.sum(axis=(1, 2)), length, rtol=1e-12, atol=0), label
    return r


# (tree, kind, k, repetitions, rep_offset, x on the longest branch or None: the forests' own sf, bins, span)
# Repetitions to a workgroup (htsamp_tile: the largest of 256, 128, 64 whose accumulators fit 136 KiB of LDS): 256 up to 67
# states, 128 up to 133, 64 up to 256 -- 67 / 68 are both sides of the first step; 65: two chunks of the pi table; 300: uint16
# states and the accumulators in HBM.  1024 repetitions: several tiles; 250, 100 and 1: a ragged tile.  caterpillar200 in 40
# bins: bins with a handful of segments, most branches cut once at the most; forest300 in 40 bins: a branch crosses up to 8.
# x = 30: many events on a branch, spread over the bins.
CASES = [
    ('forest300', 'F81', 2, 1024, 0, None, 1, 'cover'),
    ('forest300', 'F81', 4, 250, 3, None, 5, 'cover'),
    ('forest300', 'F81', 4, 1, 0, None, 5, 'middle'),
    ('forest300', 'JC', 4, 1024, 0, None, 5, 'cover'),
    ('forest300', 'F81', 64, 250, 3, None, 5, 'cover'),
    ('forest300', 'F81', 65, 250, 0, None, 1, 'cover'),
    ('forest300', 'F81', 300, 250, 3, None, 5, 'middle'),
    ('forest300', 'F81', 300, 1, 0, None, 5, 'cover'),
    ('forest300', 'F81', 4, 250, 3, 30.0, 5, 'middle'),
    ('forest300', 'F81', 4, 100, 0, 30.0, 40, 'cover'),
    ('zero64', 'F81', 4, 250, 3, None, 5, 'cover'),
    ('zero64', 'F81', 67, 250, 0, None, 5, 'cover'),
    ('zero64', 'F81', 68, 250, 3, None, 1, 'cover'),
    ('caterpillar200', 'F81', 4, 250, 3, None, 40, 'cover'),
    ('caterpillar200', 'F81', 256, 64, 0, None, 5, 'cover'),
    ('single', 'F81', 4, 250, 3, None, 1, 'cover'),
]


@pytest.mark.parametrize('tree, kind, k, n_rep, rep_offset, x_top, M, span', CASES,
                         ids=['{}-{}-k{}-r{}-M{}-{}{}'.format(c[0], c[1], c[2], c[3], c[6], c[7], '-x30' if c[5] else '') for c in CASES])
def test_histories_through_time_draw_for_draw(tree, kind, k, n_rep, rep_offset, x_top, M, span):
    flat = _forest(tree)
    model = _model(kind, k, flat, tree, x_top)
    masks = _masks(flat, k, 7 * k + 1, tree)[None]
    t, T = _times(flat, tree, M, span)
    seed = (10 << 32) + 1000 * k + n_rep + len(tree) + M
    out, E = _draw(flat, model, k, masks, t, T, n_rep, seed, rep_offset)
    assert out[0].dtype == (np.uint8 if k <= 256 else np.uint16)
    r = _check(flat, out, E, model, seed, rep_offset, t, T, '{} {} k={} n_rep={} M={} {}'.format(tree, kind, k, n_rep, M, span),
               covering=span == 'cover' and tree != 'single')
    if x_top is not None:
        assert r['events'].max() >= 30, 'no long branch in the case'
        assert (r['scale'] > 0).sum() > 100, 'hardly a branch with events is cut'
    if tree == 'zero64':
        sp = r['plan']
        zero = (flat.parent >= 0) & (t == t[np.maximum(flat.parent, 0)])
        assert zero.any() and (sp['w'][zero[sp['node']]] == 1.0).all() and sp['ends'][zero[sp['node']]].all()
    if M == 40:
        assert np.bincount(r['plan']['node']).max() >= (8 if tree == 'forest300' else 2), 'no branch crosses several bins'
    if span == 'middle':
        assert (out[3][:, 0].sum(axis=-1) > 0).all() and (out[3][:, M].sum(axis=-1) > 0).all()   # (alive at both outer boundaries)


def _engine(flat, k, model, masks, tune=None):
    eng = hip.Engine(flat, 1, k, tune=tune)
    _marginal_pass(eng, [model], masks)
    return eng


def test_against_the_whole_tree_sampler_and_the_contracts_of_a_call():
    flat = _forest('forest300')
    k, n_rep, seed = 6, 300, 31337
    model = _model('F81', k, flat, 'forest300')
    masks = _masks(flat, k, 40)[None]
    t, T = _times(flat, 'forest300', 5)
    with _engine(flat, k, model, masks) as eng:
        counts = eng.expected_counts()
        whole = eng.sample_histories_through_time(t, T, n_rep, seed)
        parent = eng.sample_histories(n_rep, seed)
        scenarios, fallen = eng.sample_scenarios(n_rep, seed)
        assert fallen == 0 and whole[4] == 0 and parent[4] == 0
        # against the parent on the device: the same scenarios, the same events, the same dwells to rounding
        assert whole[0].dtype == scenarios.dtype and np.array_equal(whole[0], scenarios)
        assert np.array_equal(whole[2].sum(axis=1, dtype=np.uint32), parent[2])
        assert np.allclose(whole[1].sum(axis=1), parent[1], rtol=1e-12, atol=0)
        assert np.array_equal(whole[3].sum(axis=-1), np.broadcast_to(ht.crossing(flat.parent, t, T), (n_rep, 6)))
        _, tau, tf = model[1]
        length = ((flat.dist[flat.parent >= 0] + tau) * tf).sum()
        assert np.allclose(whole[1].sum(axis=(1, 2)), length, rtol=1e-12, atol=0)
        # calls with rep_offset 0 / 6 / 130 make up one call, bit for bit
        parts = [eng.sample_histories_through_time(t, T, c, seed, rep_offset=o) for o, c in ((0, 6), (6, 124), (130, n_rep - 130))]
        for i, axis in enumerate((1, 0, 0, 0)):
            assert np.array_equal(np.concatenate([p[i] for p in parts], axis=axis), whole[i]), i
        # another seed gives other draws
        assert not np.array_equal(eng.sample_histories_through_time(t, T, n_rep, seed + 1, states=False)[1], whole[1])
        # what is not asked for is not computed, and times has the same bits
        for jumps, lineages, states in ((False, False, False), (False, True, True), (True, False, False)):
            got = eng.sample_histories_through_time(t, T, n_rep, seed, jumps=jumps, lineages=lineages, states=states)
            assert np.array_equal(got[1], whole[1])
            assert (got[0] is None) == (not states) and (got[2] is None) == (not jumps) and (got[3] is None) == (not lineages)
            assert _same([x for x in got[:4] if x is not None], [y for x, y in zip(got[:4], whole[:4]) if x is not None])
        # the rows of bin 2 of the five-bin call are the one-bin call on [T_2, T_3]
        one = eng.sample_histories_through_time(t, T[2:4], n_rep, seed)
        assert np.array_equal(one[1][:, 0], whole[1][:, 2]) and np.array_equal(one[2][:, 0], whole[2][:, 2])
        assert np.array_equal(one[3], whole[3][:, 2:4])
        # the results of the pass stay
        assert np.array_equal(eng.sample_scenarios(n_rep, seed)[0], scenarios)
        assert np.array_equal(eng.expected_counts(), counts)


@pytest.mark.parametrize('k', [4, 300])
def test_bits_do_not_depend_on_schedules_or_numbering(k):
    flat = _forest('forest300')
    n_rep, seed = 200, 778 + k
    model = _model('F81', k, flat, 'forest300')
    masks = _masks(flat, k, 3)[None]
    t, T = _times(flat, 'forest300', 5)
    base, _ = _draw(flat, model, k, masks, t, T, n_rep, seed)
    assert base[2].sum() > 0
    for tune in (dict(NO_HEIGHT_ORDER=1), dict(NO_SUPER=1)):   # (the caller's numbering kept; the sweeps' other schedule)
        other, _ = _draw(flat, model, k, masks, t, T, n_rep, seed, tune=tune)
        assert _same(base[:4], other[:4]), tune


def test_means_are_the_device_history_through_time():
    flat = _forest('forest300')
    k, n_rep, seed, M = 4, 4096, (3 << 32) + 101, 4
    model = _model('F81', k, flat, 'forest300', x_top=2.0)
    masks = _masks(flat, k, 29)[None]
    t, T = _times(flat, 'forest300', M)
    with _engine(flat, k, model, masks) as eng:
        exact_times, exact_jumps, exact_lineages = (x[0] for x in eng.history_through_time(t, T))
        _, times, jumps, lineages, fallen = eng.sample_histories_through_time(t, T, n_rep, seed, states=False)
    assert fallen == 0
    tested = dict(times=0, jumps=0, lineages=0)

    def hold(kind, label, column, want):
        column = column.astype(np.float64)
        se = column.std(ddof=1) / math.sqrt(n_rep)
        z = abs(column.mean() - want) / se
        print('{}{}: mean {:.6g} exact {:.6g} z {:.2f}'.format(kind, label, column.mean(), want, z))
        assert z <= BOUND, (kind, label, z)
        tested[kind] += 1

    for m in range(M):
        for s in range(k):
            if exact_times[m, s] >= 1.0:
                hold('times', (m, s), times[:, m, s], exact_times[m, s])
            for j in range(k):
                if j != s and exact_jumps[m, s, j] >= 1.0:
                    hold('jumps', (m, s, j), jumps[:, m, s, j], exact_jumps[m, s, j])
    for m in range(M + 1):
        for s in range(k):
            if exact_lineages[m, s] >= 1.0:
                hold('lineages', (m, s), lineages[:, m, s], exact_lineages[m, s])
    assert tested['times'] >= M * k and tested['lineages'] >= M + 1 and tested['jumps'] >= 4, tested


def _refused(call, status, *words):
    with pytest.raises(hip.HipError) as info:
        call()
    assert info.value.status == status, str(info.value)
    for word in words:
        assert word in str(info.value), str(info.value)
    return str(info.value)


def test_refusals_leave_the_context_answering():
    flat = _forest('zero64')
    k = 4
    name = 'pml_sample_histories_through_time'
    masks = _masks(flat, k, 5, 'forest300')[None]
    t, T = _times(flat, 'zero64', 3)
    # no marginal pass
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([_model('F81', k, flat, 'forest300')])
        eng.set_masks(masks)
        _refused(lambda: eng.sample_histories_through_time(t, T, 8, 1), hip.PML_ERR_INVALID, name + ' needs a marginal pml_bottom_up')
        eng.bottom_up(False)   # a joint sweep is not one
        _refused(lambda: eng.sample_histories_through_time(t, T, 8, 1), hip.PML_ERR_INVALID, name + ' needs a marginal pml_bottom_up')
    # a model kind other than F81
    with hip.Engine(flat, 1, 4) as eng:
        _marginal_pass(eng, [_spec('HKY', 4, flat)], masks)
        counts = eng.expected_counts()
        _refused(lambda: eng.sample_histories_through_time(t, T, 8, 1), hip.PML_ERR_UNSUPPORTED, name, 'F81', 'HKY')
        assert np.array_equal(eng.expected_counts(), counts)
    # the times and the boundaries
    with _engine(flat, k, _model('F81', k, flat, 'forest300'), masks) as eng:
        counts = eng.expected_counts()
        first = eng.sample_histories_through_time(t, T, 8, 1)
        _refused(lambda: eng.sample_histories_through_time(t, T[::-1], 8, 1), hip.PML_ERR_INVALID, name, 'ascending')
        _refused(lambda: eng.sample_histories_through_time(t, T[:1], 8, 1), hip.PML_ERR_INVALID, name, 'M = 0')
        early = t.copy()
        early[17] = early[flat.parent[17]] - 0.5
        _refused(lambda: eng.sample_histories_through_time(early, T, 8, 1), hip.PML_ERR_INVALID, name,
                 'node 17 is earlier than its parent {}'.format(flat.parent[17]))
        early[17] = np.nan
        _refused(lambda: eng.sample_histories_through_time(early, T, 8, 1), hip.PML_ERR_INVALID, name, 'node 17', 'finite')
        many = np.linspace(t.min(), t.max(), (1 << 24) // 16 + 2)
        _refused(lambda: eng.sample_histories_through_time(t, many, 1, 1, jumps=False, lineages=False, states=False),
                 hip.PML_ERR_UNSUPPORTED, name, 'PML_HIST_TIME_MAX_CELLS')
        _refused(lambda: eng.sample_histories_through_time(t, T, 0, 1), hip.PML_ERR_INVALID, name, 'n_repetitions')
        assert np.array_equal(eng.expected_counts(), counts)   # (the results of the pass stay)
        assert _same(first[:4], eng.sample_histories_through_time(t, T, 8, 1)[:4])
    # a column whose pi . pi is 1, one state
    with hip.Engine(flat, 1, 2) as eng:
        both = np.ones((1, flat.n_nodes, 2), dtype=np.int8)
        _marginal_pass(eng, [(dict(kind=hip.KIND_F81, pi=np.array([1.0, 0.0])), (1.0, 0.1, 1.0))], both)
        _refused(lambda: eng.sample_histories_through_time(t, T, 8, 1), hip.PML_ERR_INVALID, name, 'pi . pi')
    with hip.Engine(flat, 1, 1) as eng:
        _marginal_pass(eng, [(dict(kind=hip.KIND_F81, pi=np.array([1.0])), (1.0, 0.1, 1.0))], np.ones((1, flat.n_nodes, 1), dtype=np.int8))
        _refused(lambda: eng.sample_histories_through_time(t, T, 8, 1), hip.PML_ERR_INVALID, name, 'k = 1')
    # branches with x > 512
    spec, (sf, tau, tf) = _model('F81', k, flat, 'forest300')
    model = (spec, (2000.0, tau, tf))
    _, x, _ = hs.branch_scalars(flat, spec['pi'], 2000.0, tau, tf)
    n_long = int((x[flat.parent >= 0] > hs.MAX_X).sum())
    assert 0 < n_long < int((flat.parent >= 0).sum())
    with _engine(flat, k, model, masks) as eng:
        counts = eng.expected_counts()
        text = _refused(lambda: eng.sample_histories_through_time(t, T, 70, 1), hip.PML_ERR_UNSUPPORTED, name, '512')
        assert int(re.search(r'(\d+) branches', text).group(1)) == n_long, text
        assert np.array_equal(eng.expected_counts(), counts)   # (the results of the pass stay)
        assert eng.sample_scenarios(8, 1)[0].shape == (flat.n_nodes, 8)


def test_front_end_refuses_other_models_by_name():
    from pastml_amd.utilities.history_sampler import sample_histories_through_time
    flat = _forest('zero64')
    roots = flat.to_tree_nodes()
    model = HKYModel(forest_stats=ForestStats(roots), sf=1.0)
    with pytest.raises(NotImplementedError, match='HKY') as info:
        sample_histories_through_time(roots, 'c', model, 4, n_repetitions=8)
    assert 'PML_ERR_UNSUPPORTED' in str(info.value) and 'sample_histories_through_time' in str(info.value)


def test_front_end_on_the_albania_tree(monkeypatch):
    from pastml_amd.utilities.history_sampler import history_time_summary, sample_histories, sample_histories_through_time
    zz = load_golden('albania_F81')
    n_rep = 512

    def problem():
        tree = read_tree(TREE_NWK)
        preannotate_forest([tree], df=pd.read_csv(STATES_INPUT, index_col=0, header=0)[['Country']])
        f81 = F81Model(states=zz['opt_states'], forest_stats=ForestStats([tree]), sf=float(zz['opt_sf']),
                       frequencies=zz['opt_frequencies'])
        return tree, f81

    tree, f81 = problem()
    k = len(f81.states)
    np.random.seed(33)
    out = sample_histories_through_time([tree], 'Country', f81, 6, n_repetitions=n_rep)
    assert sorted(out) == ['bin_length', 'boundaries', 'jumps', 'lineages', 'states', 'times', 'tree_length']
    assert out['times'].shape == (n_rep, 6, k) and out['jumps'].shape == (n_rep, 6, k, k) and out['lineages'].shape == (n_rep, 7, k)
    assert out['jumps'].dtype == np.uint32 and out['lineages'].dtype == np.uint32
    assert out['boundaries'].shape == (7,) and out['bin_length'].shape == (6,) and list(out['states']) == list(f81.states)
    flat = ml.get_flat_forest([tree])
    dates = annotate_dates(flat)
    assert out['boundaries'][0] == dates.min() and out['boundaries'][-1] == dates[flat.tips].max()
    assert np.allclose(out['times'].sum(axis=2), out['bin_length'], rtol=1e-11, atol=1e-12 * out['tree_length'])
    assert np.allclose(out['times'].sum(axis=(1, 2)), out['tree_length'], rtol=1e-12, atol=0)
    assert np.array_equal(out['lineages'].sum(axis=-1), np.broadcast_to(ht.crossing(flat.parent, dates, out['boundaries']), (n_rep, 7)))
    # the same seed: the scenarios and the events of sample_histories
    tree1, f81_1 = problem()
    np.random.seed(33)
    parent = sample_histories([tree1], 'Country', f81_1, n_repetitions=n_rep)
    assert np.array_equal(out['jumps'].sum(axis=1, dtype=np.uint32), parent['jumps'])
    flat1 = ml.get_flat_forest([tree1])
    assert np.array_equal(np.stack([n.Country for n in flat.nodes]), np.stack([n.Country for n in flat1.nodes]))
    # a small device budget: chunks that make up the same arrays
    tree2, f81_2 = problem()
    per_rep = sample_histories_through_time.last_stats['bytes_per_repetition']
    monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(2 * per_rep * 200))
    np.random.seed(33)
    chunked = sample_histories_through_time([tree2], 'Country', f81_2, 6, n_repetitions=n_rep)
    assert sample_histories_through_time.last_stats['repetitions_per_call'] == 200
    for key in ('times', 'jumps', 'lineages'):
        assert np.array_equal(chunked[key], out[key]), key
    monkeypatch.delenv('PASTML_AMD_DEVICE_BYTES')
    # the means: the closed forms
    tree3, f81_3 = problem()
    exact = ml.expected_history_through_time([tree3], 'Country', f81_3, 6)
    assert np.array_equal(exact['boundaries'], out['boundaries'])
    s = history_time_summary(out)
    se = out['times'].std(axis=0, ddof=1) / math.sqrt(n_rep)
    # (a mean of 512 draws is normal where the state is met often: the states that hold a hundredth of their bin or more)
    held = exact['times'] >= 0.01 * out['bin_length'][:, None]
    z = np.abs(s['times']['mean'] - exact['times'])[held] / se[held]
    print('times: worst z {:.2f} over {} entries'.format(z.max(), z.size))
    assert (z <= BOUND).all() and z.size >= 12
    assert s['rates']['mean'].shape == (6, k, k) and s['rates']['kept'].max() == n_rep
    # lineages and jumps left out
    tree4, f81_4 = problem()
    np.random.seed(33)
    bare = sample_histories_through_time([tree4], 'Country', f81_4, out['boundaries'], n_repetitions=64, jumps=False, lineages=False)
    assert bare['jumps'] is None and bare['lineages'] is None and np.array_equal(bare['times'], out['times'][:64])
