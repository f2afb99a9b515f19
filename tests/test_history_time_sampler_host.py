"""Host side of sample_histories_through_time and history_time_summary (pastml_amd.utilities.history_sampler): refusals, the
passes asked for, chunking under PASTML_AMD_DEVICE_BYTES, what it returns and attaches.  No GPU: the forest problem and its
engine are replaced by stand-ins that return known arrays."""
import numpy as np
import pytest

from pastml_amd import sharding
from pastml_amd.annotation import ForestStats
from pastml_amd.ml import time_bin_fractions
from pastml_amd.models._closed_form import F81Model, JCModel
from pastml_amd.models._eigen import CustomRatesModel
from pastml_amd.tree import FlatForest, annotate_dates, get_flat_forest
from pastml_amd.utilities import history_sampler
from pastml_amd.utilities.history_sampler import history_time_summary, sample_histories_through_time


def _states(k):
    return np.array(['s{}'.format(i) for i in range(k)])


class FakeEngine(object):
    """Stands for hip.Engine: entry (node, global repetition g) of the states is (7 node + g) mod k, times[g][m][s] =
    g + m / 2 + s / 8, jumps[g][m][i][j] = g + 100 m + 3 i + j off the diagonal, lineages[g][m][s] = (g + m + s) mod 7."""
    def __init__(self, n_nodes, k):
        self.n_nodes, self.k = n_nodes, k
        self.calls = []
        self.free = 1 << 40
        self.fallen = 0

    def memory(self):
        return 0, self.free

    def sample_histories_through_time(self, node_times, boundaries, count, seed, rep_offset=0, col=0, jumps=True, lineages=True,
                                      states=True):
        self.calls.append((count, seed, rep_offset, jumps, lineages, states))
        self.node_times, self.boundaries = np.array(node_times), np.array(boundaries)
        k, M = self.k, len(boundaries) - 1
        g = rep_offset + np.arange(count)
        nodes = np.arange(self.n_nodes)[:, None]
        s = ((7 * nodes + g[None, :]) % k).astype(np.uint8 if k <= 256 else np.uint16)
        t = g[:, None, None] + np.arange(M)[None, :, None] / 2.0 + np.arange(k)[None, None, :] / 8.0
        j = (g[:, None, None, None] + 100 * np.arange(M)[None, :, None, None] + 3 * np.arange(k)[None, None, :, None] +
             np.arange(k)[None, None, None, :]).astype(np.uint32)
        j[:, :, np.arange(k), np.arange(k)] = 0
        l = ((g[:, None, None] + np.arange(M + 1)[None, :, None] + np.arange(k)[None, None, :]) % 7).astype(np.uint32)
        return (s if states else None), t, (j if jumps else None), (l if lineages else None), self.fallen


class FakeProblem(object):
    """Stands for ml.ForestProblem: records the passes it is asked for."""
    last = None

    def __init__(self, trees, character, states):
        self.flat = get_flat_forest(trees)
        self.engine = FakeEngine(self.flat.n_nodes, len(states))
        self.engine.free = FakeProblem.free
        self.engine.fallen = FakeProblem.fallen
        self.steps = []
        FakeProblem.last = self

    def initialize_allowed_states(self):
        self.steps.append('initialize')

    def alter_zero_node_allowed_states(self):
        self.steps.append('alter')

    def bottom_up_loglikelihood(self, model, is_marginal=True, alter=True):
        self.steps.append(('bottom_up', is_marginal, alter))

    def top_down_marginals(self):
        self.steps.append('top_down')

    def close(self):
        self.steps.append('close')


@pytest.fixture
def fake(monkeypatch):
    FakeProblem.free = 1 << 40
    FakeProblem.fallen = 0
    FakeProblem.last = None
    monkeypatch.setattr(history_sampler, 'ForestProblem', FakeProblem)
    monkeypatch.setattr(sharding, 'rank_world', lambda: (0, 1))
    monkeypatch.delenv('PASTML_AMD_DEVICE_BYTES', raising=False)
    return FakeProblem


def _forest(n_tips=40):
    flat = FlatForest.random(n_tips, seed=1, max_arity=4, zero_frac=0.1, n_trees=3)
    return flat.to_tree_nodes(), flat


def _f81(k=4, tau=0.0, forest_stats=None):
    return F81Model(states=_states(k), forest_stats=forest_stats, sf=1.0, frequencies=np.full(k, 1.0 / k), tau=tau)


def test_refusals(fake, monkeypatch):
    roots, _ = _forest()
    for n in (0, -3):
        with pytest.raises(ValueError, match=r'Character Country: n_repetitions must be at least 1 .*through time.*F81'):
            sample_histories_through_time(roots, 'Country', _f81(), 4, n_repetitions=n)
    with pytest.raises(ValueError, match=r'Character Host has 513 states: the MI355X history sampler supports at most 512 states '
                                         r'.*PML_ERR_UNSUPPORTED'):
        sample_histories_through_time(roots, 'Host', _f81(513), 4, n_repetitions=10)
    k = 5
    rates = np.ones((k, k)) - np.eye(k)
    cr = CustomRatesModel(forest_stats=None, sf=1.0, states=_states(k), rate_matrix=rates, frequencies=np.full(k, 1.0 / k))
    with pytest.raises(NotImplementedError, match=r'Character Host: sample_histories_through_time is for the F81 family '
                                                  r'.*CUSTOM_RATES.*PML_ERR_UNSUPPORTED'):
        sample_histories_through_time(roots, 'Host', cr, 4, n_repetitions=10)
    monkeypatch.setattr(sharding, 'rank_world', lambda: (1, 4))
    with pytest.raises(NotImplementedError, match=r'sample_histories_through_time is not supported under a multi-process launch '
                                                  r'\(4 ranks\)'):
        sample_histories_through_time(roots, 'Host', _f81(), 4, n_repetitions=10)
    assert fake.last is None   # (no problem was set up for any of them)
    monkeypatch.setattr(sharding, 'rank_world', lambda: (0, 1))
    # boundaries that are none: refused before any pass, the problem closed
    for bad in (0, [1.0], [0.0, 2.0, 1.0], [0.0, np.nan]):
        with pytest.raises(ValueError, match='time bin|boundaries'):
            sample_histories_through_time(roots, 'Host', _f81(), bad, n_repetitions=10)
        assert fake.last.steps == ['close']


def test_the_pass_the_result_and_the_attached_scenarios(fake):
    roots, flat = _forest()
    model = _f81(4, tau=0.0)
    np.random.seed(42)
    out = sample_histories_through_time(roots, 'c', model, 3, n_repetitions=37)
    problem = fake.last
    assert problem.steps == ['initialize', 'alter', ('bottom_up', True, False), 'top_down', 'close']
    assert problem.engine.calls == [(37, problem.engine.calls[0][1], 0, True, True, True)]
    n, g, k = flat.n_nodes, np.arange(37), 4
    assert sorted(out) == ['bin_length', 'boundaries', 'jumps', 'lineages', 'states', 'times', 'tree_length']
    assert list(out['states']) == list(model.states)
    # an int M: M equal bins from the earliest root to the latest tip, over annotate_dates' times, which the engine was given
    dates = annotate_dates(flat)
    assert np.array_equal(problem.engine.node_times, dates)
    assert np.array_equal(out['boundaries'], np.linspace(dates[flat.parent < 0].min(), dates[flat.tips].max(), 4))
    assert np.array_equal(problem.engine.boundaries, out['boundaries'])
    assert out['times'].shape == (37, 3, k) and out['times'][5, 2, 3] == 5 + 1.0 + 3 / 8.0
    assert out['jumps'].shape == (37, 3, k, k) and out['jumps'].dtype == np.uint32 and out['jumps'][5, 2, 2, 1] == 5 + 200 + 6 + 1
    assert out['lineages'].shape == (37, 4, k) and out['lineages'].dtype == np.uint32 and out['lineages'][5, 3, 2] == 10 % 7
    _, tau, tau_factor = model.rate_params()
    length = np.where(flat.parent >= 0, (flat.dist + tau) * tau_factor, 0.0)
    assert out['tree_length'] == pytest.approx(length.sum(), rel=1e-15)
    assert out['bin_length'].shape == (3,)
    assert np.array_equal(out['bin_length'], time_bin_fractions(flat, dates, out['boundaries']).dot(length))
    assert out['bin_length'].sum() == pytest.approx(out['tree_length'], rel=1e-12)
    # the scenarios: every node its row of one [N, n_repetitions] array, as sample_scenarios attaches them
    expected = (7 * np.arange(n)[:, None] + g[None, :]) % 4
    assert np.array_equal(np.stack([node.c for node in flat.nodes]), expected)
    assert flat.nodes[3].c.base is flat.nodes[4].c.base
    # given boundaries and root dates; tau > 0: no alteration; what is not asked for is None and not asked of the engine
    T = [1990.5, 1991.0, 1993.25]
    out = sample_histories_through_time(roots, 'c1', _f81(4, tau=0.1, forest_stats=ForestStats(roots)), T, n_repetitions=5,
                                        root_dates=[1990.0, 1990.5, 1991.0], jumps=False, lineages=False)
    assert fake.last.steps[:2] == ['initialize', ('bottom_up', True, False)]
    assert out['jumps'] is None and out['lineages'] is None and out['times'].shape == (5, 2, 4)
    assert fake.last.engine.calls[0][3:] == (False, False, True)
    assert np.array_equal(out['boundaries'], T) and np.array_equal(fake.last.engine.boundaries, T)
    assert np.array_equal(fake.last.engine.node_times, annotate_dates(flat, [1990.0, 1990.5, 1991.0]))
    # JC is of the family; a tree instead of a list
    sample_histories_through_time(flat.nodes[0], 'c', JCModel(states=_states(4), forest_stats=None, sf=1.0), 2, n_repetitions=3)
    # seeded from numpy's global generator
    np.random.seed(42)
    sample_histories_through_time(roots, 'c', model, 3, n_repetitions=8)
    first = fake.last.engine.calls[0][1]
    sample_histories_through_time(roots, 'c', model, 3, n_repetitions=8)
    assert problem.engine.calls[0][1] == first != fake.last.engine.calls[0][1]


def test_a_fallback_is_an_error(fake):
    roots, _ = _forest()
    fake.fallen = 2
    with pytest.raises(RuntimeError, match='2 draws found no state with weight'):
        sample_histories_through_time(roots, 'c', _f81(), 2, n_repetitions=8)
    assert fake.last.steps[-1] == 'close'


@pytest.mark.parametrize('k, jumps, lineages', [(4, True, True), (4, False, True), (4, True, False), (300, True, True)])
def test_chunks_by_the_device_memory(fake, monkeypatch, k, jumps, lineages):
    roots, flat = _forest(70)
    n, M = flat.n_nodes, 5
    dates = annotate_dates(flat)
    T = np.linspace(dates.min(), dates[flat.tips].max(), M + 1)
    # the segments of the plan: one per (branch with extent, bin it overlaps), one per branch without extent inside the range
    parent = flat.parent
    segments = 0
    for node in range(n):
        if parent[node] < 0:
            continue
        tp, tn = dates[parent[node]], dates[node]
        if tn == tp:
            segments += int(T[0] <= tn <= T[-1])
        else:
            segments += sum(1 for m in range(M) if min(T[m + 1], tn) > max(T[m], tp))
    assert segments > int((parent >= 0).sum()) and history_sampler._time_segments(flat, dates, T) == segments
    # per repetition: the states; the times [M, k] and one row of k partials per piece -- pieces of 64 segments here, and every
    # bin may add a ragged one --; the uint32 jump tables [M, k, k]; the uint32 lineages [M + 1, k]
    assert 64 < n <= 128
    pieces = (segments + 63) // 64 + M
    assert history_sampler._time_pieces(n, segments, M) == pieces
    assert history_sampler._time_pieces(1 << 20, 3 << 20, 16) == 3 * 256 + 16
    per_rep = (n * (1 if k <= 256 else 2) + (M + pieces) * k * 8 + (M * k * k * 4 if jumps else 0) +
               ((M + 1) * k * 4 if lineages else 0))
    assert history_sampler._bytes_per_repetition_through_time(n, k, M, segments, jumps, lineages) == per_rep
    # room for 100 repetitions per call (half of the budget goes to the call's buffers)
    monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(2 * per_rep * 100 + 17))
    out = sample_histories_through_time(roots, 'c', _f81(k), T, n_repetitions=1001, jumps=jumps, lineages=lineages)
    calls = fake.last.engine.calls
    assert [(c[0], c[2]) for c in calls] == [(100, o) for o in range(0, 1000, 100)] + [(1, 1000)]
    assert len({c[1] for c in calls}) == 1 and {c[3:] for c in calls} == {(jumps, lineages, True)}
    assert sample_histories_through_time.last_stats == dict(repetitions_per_call=100, bytes_per_repetition=per_rep)
    g = np.arange(1001)
    assert np.array_equal(out['times'][:, 1, :], g[:, None] + 0.5 + np.arange(k)[None, :] / 8.0)
    if jumps:
        assert np.array_equal(out['jumps'][:, 2, 1, 0], g + 200 + 3)
    if lineages:
        assert np.array_equal(out['lineages'][:, 5, 1], (g + 6) % 7)
    assert np.array_equal(np.stack([node.c for node in flat.nodes]), (7 * np.arange(n)[:, None] + g[None, :]) % k)
    # the engine's own free memory bounds the plan as well; never fewer than 4 repetitions per call
    monkeypatch.delenv('PASTML_AMD_DEVICE_BYTES')
    fake.free = 10
    sample_histories_through_time(roots, 'c', _f81(k), T, n_repetitions=9, jumps=jumps, lineages=lineages)
    assert [(c[0], c[2]) for c in fake.last.engine.calls] == [(4, 0), (4, 4), (1, 8)]


def test_history_time_summary():
    rng = np.random.default_rng(4)
    R, M, k = 500, 2, 3
    times = rng.gamma(3.0, 1.0, size=(R, M, k))
    jumps = rng.poisson(4.0, size=(R, M, k, k)).astype(np.uint32)
    jumps[:, :, np.arange(k), np.arange(k)] = 0
    lineages = rng.poisson(6.0, size=(R, M + 1, k)).astype(np.uint32)
    # state 2 is not visited in bin 1 in the first 100 repetitions (no jumps out of it then), state 1 never in bin 0
    times[:100, 1, 2] = 0.0
    jumps[:100, 1, 2, :] = 0
    times[:, 0, 1] = 0.0
    jumps[:, 0, 1, :] = 0
    result = dict(states=_states(k), boundaries=np.array([0.0, 1.0, 2.5]), times=times, jumps=jumps, lineages=lineages,
                  bin_length=np.array([3.0, 4.0]), tree_length=7.0)
    s = history_time_summary(result)
    assert s['level'] == 0.95 and s['n_repetitions'] == R and list(s['states']) == list(_states(k))
    assert np.array_equal(s['boundaries'], [0.0, 1.0, 2.5])
    for key, values in (('times', times), ('jumps', jumps), ('lineages', lineages)):
        values = values.astype(np.float64)
        assert s[key]['mean'].shape == values.shape[1:]
        assert np.allclose(s[key]['mean'], values.mean(axis=0))
        assert np.allclose(s[key]['lower'], np.quantile(values, 0.025, axis=0))
        assert np.allclose(s[key]['upper'], np.quantile(values, 0.975, axis=0))
    assert (s['jumps']['upper'][:, np.arange(k), np.arange(k)] == 0).all()
    # rates: jumps over dwell per repetition; a repetition with a zero dwell is left out of that entry, and counted out
    rates = s['rates']
    assert rates['mean'].shape == (M, k, k) and rates['kept'].shape == (M, k, k)
    assert (rates['kept'][0, 0] == R).all() and (rates['kept'][1, 2] == R - 100).all() and (rates['kept'][0, 1] == 0).all()
    per_rep = jumps[:, 1, 0, 1] / times[:, 1, 0]
    assert rates['mean'][1, 0, 1] == pytest.approx(per_rep.mean(), rel=1e-13)
    assert rates['lower'][1, 0, 1] == pytest.approx(np.quantile(per_rep, 0.025), rel=1e-13)
    assert rates['upper'][1, 0, 1] == pytest.approx(np.quantile(per_rep, 0.975), rel=1e-13)
    kept = jumps[100:, 1, 2, 0] / times[100:, 1, 2]
    assert rates['mean'][1, 2, 0] == pytest.approx(kept.mean(), rel=1e-13)
    assert rates['upper'][1, 2, 0] == pytest.approx(np.quantile(kept, 0.975), rel=1e-13)
    assert np.isnan(rates['mean'][0, 1]).all() and np.isnan(rates['lower'][0, 1]).all() and np.isnan(rates['upper'][0, 1]).all()
    diagonal, visited = rates['mean'][:, np.arange(k), np.arange(k)], rates['kept'][:, np.arange(k), np.arange(k)] > 0
    assert np.isfinite(rates['mean'][1]).all() and (diagonal[visited] == 0).all()
    narrow = history_time_summary(result, level=0.5)
    assert (narrow['lineages']['lower'] >= s['lineages']['lower']).all() and (narrow['times']['upper'] <= s['times']['upper']).all()
    # what the result does not hold is None
    bare = history_time_summary(dict(result, jumps=None, lineages=None))
    assert bare['jumps'] is None and bare['lineages'] is None and bare['rates'] is None and bare['times']['mean'].shape == (M, k)
    for bad in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError, match='level'):
            history_time_summary(result, level=bad)
