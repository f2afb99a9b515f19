"""Host side of simulate_states (pastml_amd.utilities.state_simulator): refusals, the column it writes, chunking.  No GPU:
the engine is replaced by a stand-in that returns known arrays."""
import numpy as np
import pytest

from pastml_amd import hip
from pastml_amd.models._closed_form import F81Model
from pastml_amd.models._eigen import CustomRatesModel
from pastml_amd.tree import FlatForest
from pastml_amd.utilities import state_simulator
from pastml_amd.utilities.state_simulator import simulate_states


def _states(k):
    return np.array(['s{}'.format(i) for i in range(k)])


class FakeEngine(object):
    """Stands for hip.Engine: simulate_states returns 7 * node + global repetition (mod 251), and records its calls."""
    calls = []
    free = 1 << 40

    def __init__(self, flat, n_cols, k, device=None):
        self.n_nodes = flat.n_nodes
        self.k = k

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def set_models(self, models):
        self.models = models

    def memory(self):
        return 0, FakeEngine.free

    def simulate_states(self, n_repetitions, seed, col=0, rep_offset=0):
        FakeEngine.calls.append((n_repetitions, seed, rep_offset))
        nodes = np.arange(self.n_nodes)[:, None]
        reps = rep_offset + np.arange(n_repetitions)[None, :]
        return ((7 * nodes + reps) % 251).astype(np.uint8)


@pytest.fixture
def fake_engine(monkeypatch):
    FakeEngine.calls = []
    FakeEngine.free = 1 << 40
    monkeypatch.setattr(hip, 'Engine', FakeEngine)
    monkeypatch.delenv('PASTML_AMD_DEVICE_BYTES', raising=False)
    return FakeEngine


def _forest():
    # ragged, several roots, polytomies
    flat = FlatForest.random(40, seed=1, max_arity=4, zero_frac=0.1, n_trees=3)
    return flat.to_tree_nodes(), flat


def test_refuses_too_few_repetitions(fake_engine):
    roots, _ = _forest()
    model = F81Model(states=_states(4), forest_stats=None, sf=1.0, frequencies=np.full(4, 0.25))
    for n in (0, -3):
        with pytest.raises(ValueError, match=r'Character Country.*F81'):
            simulate_states(roots, model, 'Country', n_repetitions=n)
    assert fake_engine.calls == []


def test_refuses_more_states_than_the_device_bound(fake_engine):
    roots, _ = _forest()
    k = 513
    model = F81Model(states=_states(k), forest_stats=None, sf=1.0, frequencies=np.full(k, 1.0 / k))
    with pytest.raises(ValueError, match=r'Character Host has 513 states.*at most 512.*F81'):
        simulate_states(roots, model, 'Host', n_repetitions=10)
    k = 257
    rates = np.ones((k, k)) - np.eye(k)
    model = CustomRatesModel(forest_stats=None, sf=1.0, states=_states(k), rate_matrix=rates, frequencies=np.full(k, 1.0 / k))
    with pytest.raises(ValueError, match=r'Character Host has 257 states.*at most 256.*CUSTOM_RATES'):
        simulate_states(roots, model, 'Host', n_repetitions=10)
    assert fake_engine.calls == []


def test_every_node_gets_its_row_of_one_array(fake_engine):
    roots, flat = _forest()
    model = F81Model(states=_states(4), forest_stats=None, sf=1.0, frequencies=np.full(4, 0.25))
    out = simulate_states(roots, model, 'sim', n_repetitions=37)
    assert out is roots
    expected = (7 * np.arange(flat.n_nodes)[:, None] + np.arange(37)[None, :]) % 251
    base = None
    for i, node in enumerate(flat.nodes):
        row = node.sim
        assert row.shape == (37,)
        assert np.array_equal(row, expected[i])
        # a view of one [N, n_repetitions] array, not an array per node
        assert row.base is not None
        base = row.base if base is None else base
        assert row.base is base
    assert base.shape == (flat.n_nodes, 37)
    # a single tree is accepted as well and returned
    one = flat.nodes[0]
    assert simulate_states(one, model, 'sim1', n_repetitions=5) is one


def test_seeded_from_numpy(fake_engine):
    roots, _ = _forest()
    model = F81Model(states=_states(4), forest_stats=None, sf=1.0, frequencies=np.full(4, 0.25))
    np.random.seed(42)
    simulate_states(roots, model, 'sim', n_repetitions=8)
    np.random.seed(42)
    simulate_states(roots, model, 'sim', n_repetitions=8)
    simulate_states(roots, model, 'sim', n_repetitions=8)
    seeds = [c[1] for c in fake_engine.calls]
    assert seeds[0] == seeds[1] != seeds[2]


def test_chunks_cover_all_repetitions(fake_engine, monkeypatch):
    roots, flat = _forest()
    model = F81Model(states=_states(4), forest_stats=None, sf=1.0, frequencies=np.full(4, 0.25))
    # room for about 100 repetitions per call (half of the budget goes to the state buffer)
    monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(2 * flat.n_nodes * 100))
    simulate_states(roots, model, 'sim', n_repetitions=1001)
    calls = fake_engine.calls
    assert len(calls) >= 3
    assert len({c[1] for c in calls}) == 1
    offset = 0
    for n, _, rep_offset in calls:
        assert rep_offset == offset
        assert n % 4 == 0 or offset + n == 1001
        offset += n
    assert offset == 1001
    expected = (7 * np.arange(flat.n_nodes)[:, None] + np.arange(1001)[None, :]) % 251
    assert np.array_equal(np.stack([n.sim for n in flat.nodes]), expected)


def test_chunks_leave_room_for_the_transition_matrices(fake_engine, monkeypatch):
    """A matrix model's first call allocates the P(t) of every branch: the chunk is planned without that memory."""
    roots, flat = _forest()
    k = 20
    rates = np.ones((k, k)) - np.eye(k)
    model = CustomRatesModel(forest_stats=None, sf=1.0, states=_states(k), rate_matrix=rates, frequencies=np.full(k, 1.0 / k))
    p_bytes = flat.n_nodes * k * 24 * 8   # (k x ks doubles per node, ks = 24)
    # room for 100 repetitions' states besides the matrices (half of what is left goes to the state buffer)
    fake_engine.free = p_bytes + 2 * flat.n_nodes * 100
    simulate_states(roots, model, 'sim', n_repetitions=1000)
    assert max(c[0] for c in fake_engine.calls) == 100
    assert sum(c[0] for c in fake_engine.calls) == 1000
