"""CPU-only: where expected_counts, marginal_counts, sample_scenarios and simulate_states let their context find P(t)
(batch.plan_consumer_window) -- the whole-tree batch whenever a column of it fits the planned memory, a window otherwise --
and what a planned window changes in the memory the repetition chunks are sized from (state_simulator._reserved_bytes).  The
budgets are computed by hand from the documented per-node and per-branch bytes; no device."""
import numpy as np
import pytest

from pastml_amd import batch, hip
from pastml_amd.tree import FlatForest
from pastml_amd.utilities import state_simulator as sim

EIGEN = hip.KIND_EIGEN


def _bytes(flat, k):
    """(the vectors of one column, one branch of the window, one column's whole-tree batch) as the planner counts them."""
    ks = k + (k & 1)
    lane = 2 if k <= 128 else 4
    lean = flat.n_nodes * (17 * ks + 96)
    per_branch = 8 * k * (-(-k // lane) * lane)
    return lean, per_branch, flat.n_nodes * per_branch


def test_materialised_when_one_column_fits():
    flat = FlatForest.random(300, seed=3, max_arity=6)
    for k in (33, 70, 130):
        lean, per_branch, full = _bytes(flat, k)
        free = (lean + full) / 0.6 + 1
        for cols in (1, 4):
            assert batch.plan_consumer_window(flat, k, EIGEN, cols, free) == 0
            assert batch.plan_consumer_window(flat, k, EIGEN, cols, free, setting='auto') == 0
            assert batch.plan_consumer_window(flat, k, EIGEN, cols, free / 100, setting='0') == 0
    # what the library has no window for: the F81 family, HKY, the eigen models up to 32 states, beyond 256
    for kind, k in ((hip.KIND_F81, 130), (hip.KIND_HKY, 4), (EIGEN, 32), (EIGEN, 20), (EIGEN, 300)):
        assert batch.plan_consumer_window(flat, k, kind, 2, 1000.0) == 0
        assert batch.plan_consumer_window(flat, k, kind, 2, 1000.0, setting='64') == 0


def test_the_largest_window_that_fits_and_the_floor_at_the_fan_out():
    flat = FlatForest.random(300, seed=3, max_arity=6)
    n, fan = flat.n_nodes, int(flat.n_children.max())
    assert fan >= 4
    k = 130
    lean, per_branch, full = _bytes(flat, k)
    # one column, room for its vectors and exactly 57 branches (and a half)
    free = (lean + 57.5 * per_branch) / 0.6
    assert batch.plan_consumer_window(flat, k, EIGEN, 1, free) == 57
    # three columns share the budget: each gets its own window of the same branches
    free = (3 * lean + 3 * 40.2 * per_branch) / 0.6
    assert batch.plan_consumer_window(flat, k, EIGEN, 3, free) == 40
    # just below a whole column: windowed, capped at the number of nodes
    free = (lean + full) / 0.6 - 1
    assert batch.plan_consumer_window(flat, k, EIGEN, 1, free) == n - 1
    # exactly the fan-out fits: the floor
    free = (lean + fan * per_branch) / 0.6
    assert batch.plan_consumer_window(flat, k, EIGEN, 1, free * (1 + 1e-12)) == fan
    # a budget that shrinks: the window shrinks down to the fan-out, never below
    last = n + 1
    for share in (0.9, 0.5, 0.2, 0.05):
        b = batch.plan_consumer_window(flat, k, EIGEN, 1, share * (lean + full) / 0.6)
        assert fan <= b <= last
        last = b
    # k = 33 .. 64: the sweeps never read P(t) there, the counts and the samplers do
    lean, per_branch, full = _bytes(flat, 40)
    assert batch.plan_consumer_window(flat, 40, EIGEN, 1, (lean + 100.5 * per_branch) / 0.6) == 100


def test_the_explicit_setting():
    flat = FlatForest.random(300, seed=3, max_arity=6)
    n, fan = flat.n_nodes, int(flat.n_children.max())
    k = 130
    lean, per_branch, full = _bytes(flat, k)
    roomy = 10 * (lean + full) / 0.6
    assert batch.plan_consumer_window(flat, k, EIGEN, 2, roomy, setting='64') == 64
    assert batch.plan_consumer_window(flat, k, EIGEN, 2, roomy, setting=' 64 ') == 64
    assert batch.plan_consumer_window(flat, k, EIGEN, 2, roomy, setting='1') == fan          # raised to the fan-out
    assert batch.plan_consumer_window(flat, k, EIGEN, 2, roomy, setting=str(10 * n)) == n    # capped at the nodes
    with pytest.raises(MemoryError) as e:
        batch.plan_consumer_window(flat, k, EIGEN, 2, (2 * lean + 2 * 63 * per_branch) / 0.6, character='host', setting='64')
    assert 'host' in str(e.value) and '64' in str(e.value) and 'PASTML_AMD_PIJ_WINDOW' in str(e.value)


def test_memory_error_names_the_character_the_states_and_the_polytomy():
    flat = FlatForest.random(300, seed=3, max_arity=6)
    fan = int(flat.n_children.max())
    k = 130
    lean, per_branch, full = _bytes(flat, k)
    free = (lean + (fan - 0.5) * per_branch) / 0.6
    for setting in (None, '64'):
        with pytest.raises(MemoryError) as e:
            batch.plan_consumer_window(flat, k, EIGEN, 1, free, character='country', setting=setting)
        assert 'country' in str(e.value) and 'k = 130' in str(e.value) and '{} branches'.format(fan) in str(e.value)
    assert batch.plan_consumer_window(flat, k, EIGEN, 1, free, character='country', setting='0') == 0   # (as before: no plan)


def test_reserved_bytes_charge_the_window_instead_of_the_batch():
    n, k = 100_000, 130
    ks = 136
    scratch = 256 << 20
    assert sim._reserved_bytes(n, k, False) == 0 and sim._reserved_bytes(n, k, False, window=64) == 0
    assert sim._reserved_bytes(n, k, True) == n * k * ks * 8 + scratch                 # as before
    assert sim._reserved_bytes(n, k, True, window=0) == sim._reserved_bytes(n, k, True)
    held = sim._reserved_bytes(n, k, True, window=512)
    assert held == 512 * k * ks * 8 + 24 * n + scratch                                 # the window and the run lists: no n k^2
    assert sim._reserved_bytes(n, 100, True, window=512) == 512 * 100 * 104 * 8 + 24 * n
    assert sim._reserved_bytes(2 * n, k, True, window=512) - held == 24 * n


def test_a_larger_chunk_is_preferred_over_a_larger_window():
    flat = FlatForest.random(300, seed=3, max_arity=6)
    n, fan = flat.n_nodes, int(flat.n_children.max())
    k = 100
    # room for everything: the window stays, one call
    free = 4 * sim._reserved_bytes(n, k, True, window=n) + 4 * n * 1000
    assert sim._window_and_chunk(flat, k, True, n, 1000, 1, free) == (n, 1000)
    assert sim._window_and_chunk(flat, k, True, 0, 1000, 1, free) == (0, 1000)
    # the planned window leaves room for 400 of 1 000 repetitions: it gives way (here down to the preferred size, which is
    # above the number of nodes' worth only if the window was: it never grows) -- and never below the fan-out
    big = FlatForest.balanced(13)
    nb = big.n_nodes
    window = 3 * batch.PIJ_WINDOW_PREFERRED
    free = sim._reserved_bytes(nb, k, True, window=window) + 2 * nb * 400
    got_window, got_chunk = sim._window_and_chunk(big, k, True, window, 1000, 1, free)
    assert got_window == batch.PIJ_WINDOW_PREFERRED
    assert got_chunk == 1000
    small = sim._reserved_bytes(nb, k, True, window=64) + 2 * nb * 400
    assert sim._window_and_chunk(big, k, True, 64, 1000, 1, small) == (64, 400)          # already below the preferred size
