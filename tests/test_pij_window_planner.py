"""CPU-only: where run_tasks lets the sweeps of a group of characters find P(t) (batch.plan_pij_window) -- the whole-tree batch
whenever a column of it fits the planned memory, a window otherwise -- with the device layer stubbed."""
import numpy as np
import pytest

from pastml_amd import batch, hip
from pastml_amd.tree import FlatForest

EIGEN = hip.KIND_EIGEN


def test_windowed_bytes_have_no_term_in_nodes_times_k_squared():
    small, large = FlatForest.balanced(6), FlatForest.balanced(9)
    for k in (100, 200):
        for widths in ([1], [k + 1]):
            lean = [batch._column_bytes(f, k, widths, kind=EIGEN, windowed=True) for f in (small, large)]
            # per node it is what an F81 column of k states costs: vectors and scalars, no k x k matrix
            assert lean == [batch._column_bytes(f, k, widths) for f in (small, large)]
            assert lean[1] / large.n_nodes == lean[0] / small.n_nodes
            full = batch._column_bytes(large, k, widths, kind=EIGEN)
            assert full - lean[1] >= large.n_nodes * 8 * k * k
    # the window: a matrix of k rows padded to the sweeps' lane width, in the character's context and, beyond 128 states (where
    # the optimiser's sum sweeps read P(t) too), in each optimiser column
    assert batch._window_bytes_per_branch(100, [3]) == 8 * 100 * 100
    assert batch._window_bytes_per_branch(130, [0]) == 8 * 130 * 132
    assert batch._window_bytes_per_branch(130, [3]) == 8 * 130 * 132 * 4


def test_materialised_when_it_fits_and_windowed_when_not():
    flat = FlatForest.random(300, seed=3, max_arity=6)
    n, fan = flat.n_nodes, int(flat.n_children.max())
    k, widths = 130, [2, 2, 2]
    per_char = batch._column_bytes(flat, k, widths, kind=EIGEN)
    # room for two columns: the numbers of before, whatever the setting (but an explicit window)
    free = 2.5 * per_char / 0.6
    assert batch.plan_pij_window(flat, k, widths, EIGEN, 3, free) == (2, 0)
    assert batch.plan_pij_window(flat, k, widths, EIGEN, 3, free, setting='auto') == (2, 0)
    assert batch.plan_pij_window(flat, k, widths, EIGEN, 3, free, setting='0') == (2, 0)
    chunk, branches = batch.plan_pij_window(flat, k, widths, EIGEN, 3, free, setting='64')
    assert branches == 64 and chunk == 3
    # room for less than one: windowed, and the plan fits the budget
    free = 0.9 * per_char / 0.6
    chunk, branches = batch.plan_pij_window(flat, k, widths, EIGEN, 3, free)
    assert chunk >= 1 and fan <= branches <= n
    lean = batch._column_bytes(flat, k, widths, kind=EIGEN, windowed=True)
    assert chunk * (lean + branches * batch._window_bytes_per_branch(k, widths)) <= 0.6 * free
    assert (chunk + 1) * (lean + min(n, batch.PIJ_WINDOW_PREFERRED) * batch._window_bytes_per_branch(k, widths)) > 0.6 * free \
        or chunk == 3
    # PASTML_AMD_PIJ_WINDOW=0: today's numbers exactly -- one column per context, no window
    assert batch.plan_pij_window(flat, k, widths, EIGEN, 3, free, setting='0') == (1, 0)
    # an explicit window is raised to the fan-out and capped at the number of nodes
    assert batch.plan_pij_window(flat, k, widths, EIGEN, 3, free, setting='1')[1] == fan
    assert batch.plan_pij_window(flat, k, widths, EIGEN, 3, 100 * free, setting=str(10 * n))[1] == n
    # what the window is not for: the F81 family, the eigen models whose sweeps never read P(t)
    for kind, kk in ((hip.KIND_F81, 130), (EIGEN, 64), (EIGEN, 20)):
        pc = batch._column_bytes(flat, kk, widths, kind=kind)
        assert batch.plan_pij_window(flat, kk, widths, kind, 3, 0.5 * pc / 0.6) == (1, 0)
    # a budget that shrinks: the window shrinks down to the fan-out, never below
    last = n + 1
    for share in (0.9, 0.5, 0.2, 0.1):
        b = batch.plan_pij_window(flat, k, widths, EIGEN, 1, share * per_char / 0.6)[1]
        assert fan <= b <= last
        last = b


def test_memory_error_names_the_character_and_the_polytomy():
    flat = FlatForest.random(300, seed=3, max_arity=6)
    fan = int(flat.n_children.max())
    k, widths = 130, [2]
    lean = batch._column_bytes(flat, k, widths, kind=EIGEN, windowed=True)
    free = (lean + (fan - 1) * batch._window_bytes_per_branch(k, widths)) / 0.6
    with pytest.raises(MemoryError, match=r'character resistance \(k = 130\).*the {} branches of the largest polytomy'.format(fan)):
        batch.plan_pij_window(flat, k, widths, EIGEN, 1, free, character='resistance')
    with pytest.raises(MemoryError, match='resistance'):
        batch.plan_pij_window(flat, k, widths, EIGEN, 1, 2 * free, character='resistance', setting=str(flat.n_nodes))
    assert batch.plan_pij_window(flat, k, widths, EIGEN, 1, free, character='resistance', setting='0') == (1, 0)


class _Model(object):
    def __init__(self, k):
        self.states = np.array(['s{}'.format(i) for i in range(k)])

    def kernel_spec(self):
        return dict(kind=EIGEN)

    def extra_params_fixed(self):
        return True

    def unfix_extra_params(self):
        pass

    def fix_extra_params(self):
        pass

    def get_num_params(self):
        return 1


def test_run_tasks_hands_the_window_to_its_batches(monkeypatch):
    """run_tasks with the device stubbed: the decision goes into its stats and onto every CharacterBatch of the group."""
    flat = FlatForest.random(300, seed=3, max_arity=6)
    k = 130
    tasks = [batch.Task('c{}'.format(i), 'MPPA', _Model(k), np.ones(k) / k) for i in range(2)]
    seen = []

    class Probe(object):
        def __init__(self, device=None):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

        def memory(self):
            return 0, 1 << 40

    monkeypatch.setattr(hip, 'BareContext', Probe)
    monkeypatch.setattr(batch, 'visible_devices', lambda device=None: [0])
    monkeypatch.setattr(batch, 'annotation_words',
                        lambda flat_, character, states: (np.zeros((flat_.n_nodes, batch.n_words(len(states))), dtype=np.uint64),
                                                          np.zeros(flat_.n_nodes, dtype=bool)))
    monkeypatch.setattr(batch, 'optimise_group', lambda b, group, seeds=None: (seen.append(b.pij_window) or np.zeros(len(group)), 0))
    monkeypatch.setattr(batch, 'reconstruct', lambda b, group, lnl, force_joint=True: [dict(character=t.character) for t in group])
    monkeypatch.setenv('PASTML_AMD_CONCURRENT_GROUPS', '0')
    widths = [batch.block_width(t.model) for t in tasks]
    per_char = batch._column_bytes(flat, k, widths, kind=EIGEN)

    def run(device_bytes, setting):
        del seen[:]
        monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(int(device_bytes)))
        if setting is None:
            monkeypatch.delenv('PASTML_AMD_PIJ_WINDOW', raising=False)
        else:
            monkeypatch.setenv('PASTML_AMD_PIJ_WINDOW', setting)
        out = batch.run_tasks(None, tasks, flat=flat, seeds=[1, 2])
        assert [r['character'] for r in out] == ['c0', 'c1']
        return batch.run_tasks.last_stats['pij_window'], list(seen)

    stats, windows = run(10 * per_char, None)
    assert stats == [dict(k=k, characters=2, mode='materialised', branches=0, characters_per_context=2)] and windows == [0]
    stats, windows = run(0.9 * per_char / 0.6, None)
    assert len(stats) == 1 and stats[0]['mode'] == 'windowed' and stats[0]['branches'] >= int(flat.n_children.max())
    assert windows == [stats[0]['branches']] * len(windows) and len(windows) == -(-2 // stats[0]['characters_per_context'])
    stats, windows = run(0.9 * per_char / 0.6, '0')
    assert stats == [dict(k=k, characters=2, mode='materialised', branches=0, characters_per_context=1)] and windows == [0, 0]
