"""Host side of sample_histories and history_summary (pastml_amd.utilities.history_sampler): refusals, chunking under
PASTML_AMD_DEVICE_BYTES, what it returns and attaches.  No GPU: the forest problem and its engine are replaced by stand-ins
that return known arrays."""
import numpy as np
import pytest

from pastml_amd import sharding
from pastml_amd.annotation import ForestStats
from pastml_amd.models._closed_form import F81Model, JCModel
from pastml_amd.models._eigen import CustomRatesModel
from pastml_amd.tree import FlatForest, get_flat_forest
from pastml_amd.utilities import history_sampler
from pastml_amd.utilities.history_sampler import history_summary, sample_histories


def _states(k):
    return np.array(['s{}'.format(i) for i in range(k)])


class FakeEngine(object):
    """Stands for hip.Engine: entry (node, global repetition g) of the states is (7 node + g) mod k, times[g][s] = g + s / 8,
    jumps[g][i][j] = g + 3 i + j off the diagonal, branch_jumps[node][g] = (node + g) mod 5."""
    def __init__(self, n_nodes, k):
        self.n_nodes, self.k = n_nodes, k
        self.calls = []
        self.free = 1 << 40
        self.fallen = 0

    def memory(self):
        return 0, self.free

    def sample_histories(self, count, seed, rep_offset=0, col=0, jumps=True, branch_jumps=False, states=True):
        self.calls.append((count, seed, rep_offset, jumps, branch_jumps, states))
        k = self.k
        g = rep_offset + np.arange(count)
        nodes = np.arange(self.n_nodes)[:, None]
        s = ((7 * nodes + g[None, :]) % k).astype(np.uint8 if k <= 256 else np.uint16)
        t = g[:, None] + np.arange(k)[None, :] / 8.0
        j = (g[:, None, None] + 3 * np.arange(k)[None, :, None] + np.arange(k)[None, None, :]).astype(np.uint32)
        j[:, np.arange(k), np.arange(k)] = 0
        b = ((nodes + g[None, :]) % 5).astype(np.uint16)
        return (s if states else None), t, (j if jumps else None), (b if branch_jumps else None), self.fallen


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
        with pytest.raises(ValueError, match=r'Character Country: n_repetitions must be at least 1 .*F81'):
            sample_histories(roots, 'Country', _f81(), n_repetitions=n)
    with pytest.raises(ValueError, match=r'Character Host has 513 states: the MI355X history sampler supports at most 512 states '
                                         r'.*PML_ERR_UNSUPPORTED'):
        sample_histories(roots, 'Host', _f81(513), n_repetitions=10)
    k = 5
    rates = np.ones((k, k)) - np.eye(k)
    cr = CustomRatesModel(forest_stats=None, sf=1.0, states=_states(k), rate_matrix=rates, frequencies=np.full(k, 1.0 / k))
    with pytest.raises(NotImplementedError, match=r'Character Host: sample_histories is for the F81 family .*CUSTOM_RATES.*'
                                                  r'PML_ERR_UNSUPPORTED'):
        sample_histories(roots, 'Host', cr, n_repetitions=10)
    monkeypatch.setattr(sharding, 'rank_world', lambda: (1, 4))
    with pytest.raises(NotImplementedError, match=r'sample_histories is not supported under a multi-process launch \(4 ranks\)'):
        sample_histories(roots, 'Host', _f81(), n_repetitions=10)
    assert fake.last is None   # (no problem was set up for any of them)


def test_the_pass_the_result_and_the_attached_scenarios(fake):
    roots, flat = _forest()
    model = _f81(4, tau=0.0)
    np.random.seed(42)
    out = sample_histories(roots, 'c', model, n_repetitions=37, branch_jumps=True)
    problem = fake.last
    assert problem.steps == ['initialize', 'alter', ('bottom_up', True, False), 'top_down', 'close']
    assert problem.engine.calls == [(37, problem.engine.calls[0][1], 0, True, True, True)]
    n, g = flat.n_nodes, np.arange(37)
    assert sorted(out) == ['branch_jumps', 'jumps', 'states', 'times', 'tree_length']
    assert list(out['states']) == list(model.states)
    assert out['times'].shape == (37, 4) and np.array_equal(out['times'], g[:, None] + np.arange(4)[None, :] / 8.0)
    assert out['jumps'].shape == (37, 4, 4) and out['jumps'].dtype == np.uint32 and out['jumps'][5, 2, 1] == 5 + 6 + 1
    assert out['branch_jumps'].shape == (n, 37) and out['branch_jumps'].dtype == np.uint16
    _, tau, tau_factor = model.rate_params()
    assert out['tree_length'] == pytest.approx(((flat.dist[flat.parent >= 0] + tau) * tau_factor).sum(), rel=1e-15)
    # the scenarios: every node its row of one [N, n_repetitions] array, as sample_scenarios attaches them
    expected = (7 * np.arange(n)[:, None] + g[None, :]) % 4
    assert np.array_equal(np.stack([node.c for node in flat.nodes]), expected)
    assert flat.nodes[3].c.base is flat.nodes[4].c.base
    # tau > 0: no alteration; a tree instead of a list; no branch counts unless asked for
    one = flat.nodes[0]
    out = sample_histories(one, 'c1', _f81(4, tau=0.1, forest_stats=ForestStats(roots)), n_repetitions=5)
    assert fake.last.steps[:2] == ['initialize', ('bottom_up', True, False)] and out['branch_jumps'] is None
    assert fake.last.engine.calls[0][3:] == (True, False, True)
    # JC is of the family
    sample_histories(roots, 'c', JCModel(states=_states(4), forest_stats=None, sf=1.0), n_repetitions=3)
    # seeded from numpy's global generator
    np.random.seed(42)
    sample_histories(roots, 'c', model, n_repetitions=8)
    first = fake.last.engine.calls[0][1]
    sample_histories(roots, 'c', model, n_repetitions=8)
    assert problem.engine.calls[0][1] == first != fake.last.engine.calls[0][1]


def test_a_fallback_is_an_error(fake):
    roots, _ = _forest()
    fake.fallen = 2
    with pytest.raises(RuntimeError, match='2 draws found no state with weight'):
        sample_histories(roots, 'c', _f81(), n_repetitions=8)
    assert fake.last.steps[-1] == 'close'


@pytest.mark.parametrize('k, branch_jumps', [(4, False), (4, True), (300, False)])
def test_chunks_by_the_device_memory(fake, monkeypatch, k, branch_jumps):
    roots, flat = _forest(70)
    n = flat.n_nodes
    # per repetition: the states, the times and one row of partials per piece (pieces of 64 ids here: two), the uint32 jump
    # table, the uint16 branch counts
    assert 64 < n <= 128 and history_sampler._pieces(n) == 2 and history_sampler._pieces(64) == 1
    assert history_sampler._pieces(256 * 64 + 1) == 129 and history_sampler._pieces(1 << 20) == 256
    per_rep = n * (1 if k <= 256 else 2) + 3 * k * 8 + k * k * 4 + (2 * n if branch_jumps else 0)
    assert history_sampler._bytes_per_repetition(n, k, branch_jumps) == per_rep
    # room for 100 repetitions per call (half of the budget goes to the call's buffers)
    monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(2 * per_rep * 100 + 17))
    out = sample_histories(roots, 'c', _f81(k), n_repetitions=1001, branch_jumps=branch_jumps)
    calls = fake.last.engine.calls
    assert [(c[0], c[2]) for c in calls] == [(100, o) for o in range(0, 1000, 100)] + [(1, 1000)]
    assert len({c[1] for c in calls}) == 1
    assert sample_histories.last_stats == dict(repetitions_per_call=100, bytes_per_repetition=per_rep)
    g = np.arange(1001)
    assert np.array_equal(out['times'], g[:, None] + np.arange(k)[None, :] / 8.0)
    assert np.array_equal(out['jumps'][:, 1, 0], g + 3)
    assert np.array_equal(np.stack([node.c for node in flat.nodes]), (7 * np.arange(n)[:, None] + g[None, :]) % k)
    if branch_jumps:
        assert np.array_equal(out['branch_jumps'], (np.arange(n)[:, None] + g[None, :]) % 5)
    # the engine's own free memory bounds the plan as well; never fewer than 4 repetitions per call
    monkeypatch.delenv('PASTML_AMD_DEVICE_BYTES')
    fake.free = 10
    sample_histories(roots, 'c', _f81(k), n_repetitions=9, branch_jumps=branch_jumps)
    assert [(c[0], c[2]) for c in fake.last.engine.calls] == [(4, 0), (4, 4), (1, 8)]


def test_history_summary():
    rng = np.random.default_rng(4)
    times = rng.gamma(3.0, 1.0, size=(500, 3))
    jumps = rng.poisson(4.0, size=(500, 3, 3)).astype(np.uint32)
    jumps[:, np.arange(3), np.arange(3)] = 0
    result = dict(states=_states(3), times=times, jumps=jumps, branch_jumps=None, tree_length=12.5)
    s = history_summary(result)
    assert s['level'] == 0.95 and s['n_repetitions'] == 500 and list(s['states']) == list(_states(3))
    assert np.allclose(s['times']['mean'], times.mean(axis=0))
    assert np.allclose(s['times']['lower'], np.quantile(times, 0.025, axis=0))
    assert np.allclose(s['times']['upper'], np.quantile(times, 0.975, axis=0))
    assert s['jumps']['mean'].shape == (3, 3) and np.allclose(s['jumps']['mean'], jumps.mean(axis=0))
    assert np.allclose(s['jumps']['upper'], np.quantile(jumps.astype(float), 0.975, axis=0))
    assert (np.diag(s['jumps']['upper']) == 0).all()
    assert np.allclose(s['time_share']['mean'], times.mean(axis=0) / 12.5)
    inside = ((times >= s['times']['lower']) & (times <= s['times']['upper'])).mean(axis=0)
    assert (np.abs(inside - 0.95) < 0.01).all()
    narrow = history_summary(result, level=0.5)
    assert (narrow['times']['lower'] > s['times']['lower']).all() and (narrow['times']['upper'] < s['times']['upper']).all()
    for bad in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError, match='level'):
            history_summary(result, level=bad)
