"""
The entries that read P(t) outside the sweeps on a context with a window of it (``-m gpu``; csrc/pml_pij_window.h):
pml_expected_counts, pml_marginal_counts(_altered), pml_simulate_states and pml_sample_scenarios build their matrices run by
run into the window and must leave what they leave on a context that keeps P(t) of every branch -- the exact counts bit for
bit (the order of every sum is fixed by the pieces of 128 ids, which do not move), the sampled counts and the scenarios
element for element (a draw is a function of seed, node and repetition) -- while the whole-tree batch is never allocated and
the memory the context holds after a call is what it held before.

Shapes: k = 33, 70 and 130 (expected_matrix_kernel<1>, <2>, <4>; one, two and three mask words; cumulative rows in LDS and, at
130, in scratch), three columns, a forest of two trees with 450 - 700 nodes (at least four pieces of ids, the last one
partial), polytomies up to arity 5, a twentieth of the internal branches of length zero, and in one tree a spine deeper than
20 levels below which subtrees of differing sizes hang, so that the frontier depth of the simulator's schedule (16) is passed:
the level runs, the groups of frontier subtrees and, at the smallest window, the moved frontier are all executed.  Windows: the
largest fan-out (below one piece of ids and below the largest frontier subtree), 200 (one piece and a remainder, several
groups) and the number of nodes (one run).  Against something other than the library: the windowed exact counts at k = 130
against tests/expected_counts_ref.py on the oracle's sweeps.  The front ends -- expected_counts, marginal_counts,
sample_scenarios, simulate_states -- with less planned memory than one column's batch takes: they report a window, return
what they return with PASTML_AMD_PIJ_WINDOW=0, and raise MemoryError where not even the smallest window fits.
"""
import numpy as np
import pytest

from pastml_amd import hip
from pastml_amd.tree import FlatForest, TreeNode
from test_gpu_parity import random_masks, random_spec
from test_gpu_pij_window import TUNES

pytestmark = pytest.mark.gpu

C = 3
FRONTIER = 16   # PML_SIM_MAX_TOP (pml_launch_simulate.hip): with so few nodes per level the schedule's frontier depth is this one
SEED = 0x5eed1234abcd


def _grow(node, n_tips, rng, max_arity):
    leaves = [node]
    while len(leaves) < n_tips:
        leaf = leaves.pop(int(rng.integers(len(leaves))))
        for _ in range(int(rng.integers(2, max_arity + 1))):
            leaves.append(leaf.add_child(dist=float(rng.uniform(0.01, 0.3))))


def spine_forest(seed):
    """Two trees: a spine of 28 nodes with a subtree of 1 .. 14 tips hanging at each of them (one or two beside the next spine
    node: arity up to 3 there, up to 5 inside the subtrees), and a ragged tree of 60 tips with polytomies up to arity 5.  A
    twentieth of the internal branches have length zero (internal ones only, and the masks leave the internal nodes free: see
    test_gpu_pij_window.ragged_forest)."""
    rng = np.random.default_rng(seed)
    first = TreeNode(name='', dist=0.0)
    at = first
    for level in range(28):
        for _ in range(int(rng.integers(1, 3))):
            sub = at.add_child(dist=float(rng.uniform(0.01, 0.3)))
            tips = int(rng.integers(1, 15))
            if tips > 1:
                _grow(sub, tips, rng, 5)
        at = at.add_child(dist=float(rng.uniform(0.01, 0.3)))
    _grow(at, 6, rng, 3)
    second = TreeNode(name='', dist=0.0)
    _grow(second, 60, rng, 5)
    grown = FlatForest.from_trees([first, second])
    dist = grown.dist.copy()
    inner = np.flatnonzero((grown.n_children > 0) & (grown.parent >= 0))
    dist[rng.choice(inner, size=max(1, len(inner) // 20), replace=False)] = 0.0
    return FlatForest(grown.parent, grown.n_children, grown.first_child, dist, grown.roots)


def _subtree_sizes(flat):
    size = np.ones(flat.n_nodes, dtype=np.int64)
    for n in range(flat.n_nodes - 1, -1, -1):   # (level order: a child's id is above its parent's)
        if flat.parent[n] >= 0:
            size[flat.parent[n]] += size[n]
    return size


_CASES = {}


def case(k):
    """(forest, specs, rates, masks, altered flags) of the k-state case: made once."""
    if k not in _CASES:
        rng = np.random.default_rng(7000 + k)
        flat = spine_forest(seed=11)
        specs = [random_spec('EIGEN', k, rng) for _ in range(C)]
        rates = [(float(rng.uniform(0.3, 4)), float(rng.choice([0.0, 0.02])), float(rng.uniform(0.7, 1.0))) for _ in range(C)]
        masks = np.stack([random_masks(flat, k, rng, missing=0.1, multi=0.1, internal=0.0) for _ in range(C)])
        altered = np.zeros(flat.n_nodes, dtype=np.uint8)
        inner = np.flatnonzero((flat.n_children > 0) & (flat.parent >= 0))
        altered[rng.choice(inner, size=5, replace=False)] = 1
        _CASES[k] = (flat, specs, rates, masks, altered)
    return _CASES[k]


def test_the_forest_has_the_shape_the_runs_need():
    flat = case(33)[0]
    size = _subtree_sizes(flat)
    fan = int(flat.n_children.max())
    assert len(flat.roots) == 2 and 450 <= flat.n_nodes <= 700 and 3 <= fan <= 5
    assert flat.n_nodes > 3 * 128 and flat.n_nodes % 128 != 0                   # at least four pieces, the last one partial
    assert np.count_nonzero((flat.dist == 0) & (flat.parent >= 0) & (flat.n_children > 0)) >= 5
    assert flat.n_td_levels > 20                                                # the spine
    frontier = np.flatnonzero(flat.depth == FRONTIER)
    assert len(frontier) >= 3 and len(set(size[frontier])) >= 2                 # subtrees of differing sizes hang there
    assert size[frontier].max() > fan                                           # the smallest window moves the frontier
    below = int(size[frontier].sum())
    assert below > 200 or size[frontier].max() > 200                            # window 200: several groups or a moved frontier
    assert fan < 128 < 200 < 2 * 128 < flat.n_nodes


def consumers(k, window):
    """Every result of the entries that read P(t) outside the sweeps, as raw arrays; window: None (materialised) or branches.
    On a windowed engine the batch must never be allocated and every call must give back what it took."""
    flat, specs, rates, masks, altered = case(k)
    out = {}
    with hip.Engine(flat, C, k, tune=TUNES[k]) as eng:
        eng.set_models(list(zip(specs, rates)))
        eng.set_masks(masks)
        if window is not None:
            eng.pij_window_set(window)

        def call(name, fn):
            held = eng.memory()[0]
            got = fn()
            if window is not None:
                assert eng.pij_window_info()[2] == 0, '{}: the whole-tree batch was allocated'.format(name)
                assert eng.memory()[0] == held, '{}: the context holds {} bytes, {} before'.format(name, eng.memory()[0], held)
            for i, a in enumerate(got if isinstance(got, tuple) else (got,)):
                out['{}[{}]'.format(name, i)] = np.asarray(a)

        # the simulator needs no sweep: first, on a context that has prepared nothing
        call('simulate 5 col 0', lambda: eng.simulate_states(5, SEED, col=0))
        eng.marginal_pass(posterior=False, lh=False)
        call('simulate 5 col 0 after the pass', lambda: eng.simulate_states(5, SEED, col=0))
        call('simulate 1100 col 2', lambda: eng.simulate_states(1100, SEED + 1, col=2, rep_offset=7))
        call('expected all', lambda: eng.expected_counts(0, C))
        call('expected altered', lambda: eng.expected_counts(1, 2, altered=altered))
        call('marginal counts', lambda: eng.marginal_counts(300, SEED + 2, col=1))
        call('marginal counts altered', lambda: eng.marginal_counts_altered(300, SEED + 3, altered, col=1))
        call('scenarios 5 col 0', lambda: eng.sample_scenarios(5, SEED + 4, col=0))
        call('scenarios 1100 col 2', lambda: eng.sample_scenarios(1100, SEED + 5, rep_offset=1001, col=2))
        call('scenarios 1100 col 0', lambda: eng.sample_scenarios(1100, SEED + 6, col=0))
        out['info'] = np.asarray(eng.pij_window_info())
    return out


_MATERIALISED = {}


def materialised(k):
    if k not in _MATERIALISED:
        _MATERIALISED[k] = consumers(k, None)
    return _MATERIALISED[k]


@pytest.mark.parametrize('which', ['fanout', '200', 'nodes'])
@pytest.mark.parametrize('k', [33, 70, 130])
def test_windowed_consumers_leave_what_the_materialised_ones_leave(k, which):
    flat = case(k)[0]
    window = {'fanout': int(flat.n_children.max()), '200': 200, 'nodes': flat.n_nodes}[which]
    want, got = materialised(k), consumers(k, window)
    assert want['info'][0] == 0 and want['info'][2] > 0            # the batch, no window
    assert got['info'][0] == window and got['info'][2] == 0        # the window, and the batch never was
    assert sorted(want) == sorted(got)
    for name in sorted(want):
        if name == 'info':
            continue
        assert want[name].dtype == got[name].dtype and want[name].shape == got[name].shape, name
        assert np.array_equal(want[name], got[name], equal_nan=True), name
    # (what was compared is something: finite counts, scenarios that move, no draw without weight)
    assert np.all(np.isfinite(want['expected all[0]'])) and want['expected all[0]'].shape == (C, k, k)
    assert want['expected altered[1]'].any()
    assert want['marginal counts[0]'].sum() > 0 and want['marginal counts altered[1]'].sum() > 0
    assert len(np.unique(want['scenarios 1100 col 2[0]'])) > 5 and len(np.unique(want['simulate 1100 col 2[0]'])) > 5
    for name in ('scenarios 5 col 0[1]', 'scenarios 1100 col 2[1]', 'scenarios 1100 col 0[1]'):
        assert want[name] == 0 and got[name] == 0, name
    assert np.array_equal(want['simulate 5 col 0[0]'], want['simulate 5 col 0 after the pass[0]'])


def test_windowed_exact_counts_k130_against_the_restatement():
    """Not the library against itself: the exact counts of a windowed k = 130 context (a window of 200 branches: two runs of one
    piece, ..., the last one partial) against the restatement on the oracle's sweeps, at test_gpu_expected_counts' tolerance for
    the matrix models."""
    from test_gpu_expected_counts import _assert_close, _restated
    k = 130
    flat, specs, rates, masks, _ = case(k)
    with hip.Engine(flat, C, k) as eng:
        eng.set_models(list(zip(specs, rates)))
        eng.set_masks(masks)
        eng.pij_window_set(200)
        eng.marginal_pass(posterior=False, lh=False)
        got = eng.expected_counts(1, 2)[0]
        assert eng.pij_window_info()[2] == 0
    want = _restated(flat, masks[1], specs[1], rates[1])
    assert not np.isnan(got).any()
    _assert_close(got, want['counts'], flat.n_nodes - len(flat.roots), 'windowed CR k=130')


# ---------------------------------------------------------------------------------------------------------------------
# the front ends
# ---------------------------------------------------------------------------------------------------------------------

def _annotated_cr(k=130, n_tips=120, seed=77):
    """A fresh tree with observed tips and a CUSTOM_RATES model of k states; tau > 0: no node is altered."""
    from pastml_amd.annotation import ForestStats
    from pastml_amd.models._eigen import CustomRatesModel
    flat = FlatForest.random(n_tips, seed=seed, max_arity=4, lo=0.02, hi=0.4)
    roots = flat.to_tree_nodes()
    rng = np.random.default_rng(seed + 100)
    states = np.array(['s{:03d}'.format(i) for i in range(k)])
    r = np.triu(rng.uniform(0.2, 2.0, size=(k, k)), 1)
    model = CustomRatesModel(states=states, forest_stats=ForestStats(roots), sf=1.5, tau=0.01,
                             frequencies=rng.dirichlet(np.ones(k) * 5), rate_matrix=r + r.T)
    for t in flat.tips:
        if rng.random() < 0.9:
            flat.nodes[t].add_feature('c', {states[int(rng.integers(12))]})
    model.freeze()
    return flat, roots, model


def _front_ends():
    from pastml_amd import ml
    from pastml_amd.utilities.scenario_sampler import sample_scenarios
    from pastml_amd.utilities.state_simulator import simulate_states

    def states_of(flat, name):
        return np.stack([np.asarray(getattr(flat.nodes[i], name)) for i in range(flat.n_nodes)])

    def run_expected(flat, roots, model):
        return ml.expected_counts(roots, 'c', model)

    def run_marginal(flat, roots, model):
        return ml.marginal_counts(roots, 'c', model, n_repetitions=200)

    def run_scenarios(flat, roots, model):
        sample_scenarios(roots, 'c', model, n_repetitions=37)
        return states_of(flat, 'c')

    def run_simulate(flat, roots, model):
        simulate_states(roots, model, 'sim', n_repetitions=37)
        return states_of(flat, 'sim')

    return [(ml.expected_counts, run_expected), (ml.marginal_counts, run_marginal), (sample_scenarios, run_scenarios),
            (simulate_states, run_simulate)]


@pytest.mark.parametrize('which', range(4), ids=['expected_counts', 'marginal_counts', 'sample_scenarios', 'simulate_states'])
def test_front_ends_run_windowed_when_the_batch_does_not_fit(which, monkeypatch):
    from pastml_amd import batch as B
    function, run = _front_ends()[which]
    flat = _annotated_cr()[0]
    k, fan = 130, int(flat.n_children.max())
    # less than one materialised column takes (0.6 of it is planned): as test_acr_runs_windowed_when_the_batch_does_not_fit
    one_column = int(B._column_bytes(flat, k, [0], kind=hip.KIND_EIGEN))
    lean, per_branch = B._column_bytes(flat, k, [0], kind=hip.KIND_EIGEN, windowed=True), B._window_bytes_per_branch(k, [0])
    assert 0.6 * one_column < lean + flat.n_nodes * per_branch and lean + 36 * per_branch < 0.6 * one_column
    results = {}
    try:
        for setting in (None, '0'):
            hip.drain_engine_pool()
            monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(one_column))
            if setting is None:
                monkeypatch.delenv('PASTML_AMD_PIJ_WINDOW', raising=False)
            else:
                monkeypatch.setenv('PASTML_AMD_PIJ_WINDOW', setting)
            fresh, roots, model = _annotated_cr()
            np.random.seed(99)
            results[setting] = (np.asarray(run(fresh, roots, model)), function.last_stats['pij_window'])
        # a budget below the window of the largest fan-out: refused before any device work, and the character is named
        monkeypatch.delenv('PASTML_AMD_PIJ_WINDOW', raising=False)
        monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(int((lean + (fan - 1) * per_branch) / 0.6)))
        fresh, roots, model = _annotated_cr()
        launches = []
        monkeypatch.setattr(hip.Engine, 'set_models', lambda self, *a, **kw: launches.append('set_models'))
        with pytest.raises(MemoryError, match='character (c|sim) .*k = 130'):
            run(fresh, roots, model)
        assert launches == []
    finally:
        hip.drain_engine_pool()
    (windowed, stats_w), (plain, stats_0) = results[None], results['0']
    assert len(stats_w) == 1 and stats_w[0]['mode'] == 'windowed' and stats_w[0]['k'] == k
    assert fan <= stats_w[0]['branches'] < flat.n_nodes
    assert len(stats_0) == 1 and stats_0[0]['mode'] == 'materialised' and stats_0[0]['branches'] == 0
    assert windowed.dtype == plain.dtype and windowed.shape == plain.shape and np.array_equal(windowed, plain)
    assert np.all(np.isfinite(windowed.astype(np.float64))) and len(np.unique(windowed)) > 3
