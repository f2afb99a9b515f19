"""
The horizontal merging on the device (pml_compress_horizontal, pastml_amd.visualisation.tree_compressor) against the
reference's lines (tests/golden/compress_horizontal.npz) and, on built inputs, against the host restatement -- which
test_compress_horizontal_host.py pins to the same goldens.  Every device pass in this file is compared with
``horizontal_pass_host`` on survivors, liveness and widths.  Integer work: every comparison is exact.
"""
import numpy as np
import pytest

from pastml_amd import hip, synthetic
from pastml_amd.batch import one_hot_words
from pastml_amd.tree import FlatForest
from pastml_amd.visualisation import tree_compressor as tc
from test_compress_horizontal_host import CASES, check_against_golden, load_case
from test_gpu_compress import caterpillar

pytestmark = pytest.mark.gpu


class CheckedEngine(object):
    """An engine whose every horizontal pass is compared with the host restatement."""

    def __init__(self, engine):
        self.engine = engine
        self.passes = 0
        self.infos = []

    def compress_vertical(self, *args):
        return self.engine.compress_vertical(*args)

    def compress_horizontal(self, parent, rank, bins, width, live, sets):
        device = self.engine.compress_horizontal(parent, rank, bins, width, live, sets)
        host = tc.horizontal_pass_host(parent, rank, bins, width, live, sets)
        for name, d, h in zip(('into', 'live', 'width'), device, host):
            assert d.dtype == h.dtype and np.array_equal(d, h), name
        assert device[3] == host[3]
        self.passes += 1
        self.infos.append(self.engine.compress_horizontal_info())
        return device


def device_pass(parent, bins, sets, width=None, live=None, rank=None, engine=None):
    """One pass over a vertex forest given as arrays, on the device, compared with the host: (into, live, width, groups, info)."""
    V = len(parent)
    width = np.ones(V, dtype=np.int32) if width is None else width
    live = np.ones(V, dtype=bool) if live is None else live
    rank = np.arange(V) if rank is None else rank
    if engine is None:
        with hip.Engine.tree_only(FlatForest.balanced(2)) as eng:   # (the context supplies the device and the stream, no more)
            checked = CheckedEngine(eng)
            return checked.compress_horizontal(parent, rank, bins, width, live, sets) + (checked.infos[0],)
    checked = CheckedEngine(engine)
    return checked.compress_horizontal(parent, rank, bins, width, live, sets) + (checked.infos[0],)


# ---------------------------------------------------------------------------------------------------------------------
# 1. device = reference
@pytest.mark.parametrize('case', CASES)
def test_device_reproduces_the_reference(case, tmp_path):
    flat, columns, column2states, expected = load_case(case)
    with hip.Engine.tree_only(flat) as eng:
        checked = CheckedEngine(eng)
        merged = tc.compress_forest(flat, columns, column2states, timing=tc.HORIZONTAL,
                                    tip_size_threshold=int(expected['threshold']), engine=checked)
    assert checked.passes == 1 + int((expected['passes'] == 2).any())
    check_against_golden(merged, columns, expected, tmp_path)
    host = tc.compress_forest(flat, columns, column2states, timing=tc.HORIZONTAL, tip_size_threshold=int(expected['threshold']),
                              device=False)
    for field in ('vertex', 'width', 'parent', 'members', 'member_offsets', 'n_tips_total', 'second_pass'):
        assert np.array_equal(getattr(merged, field), getattr(host, field)), field
    assert merged.merged_groups == host.merged_groups
    # ... and with a context of the module's own making
    own = tc.compress_forest(flat, columns, column2states, timing=tc.HORIZONTAL, tip_size_threshold=int(expected['threshold']),
                             device=True)
    assert tc.pajek_lines(own, columns) == tc.pajek_lines(host, columns)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the order of the children does not matter, at any arity
def sort_tile():
    with hip.Engine.tree_only(FlatForest.balanced(2)) as eng:
        return eng.compress_horizontal_info()['sort_tile']


def two_stars(n, k):
    """Root 0, stars 1 and 2, n leaves each with n distinct (col0, col1) combinations of k states; star 2 lists them reversed."""
    assert k * k >= n and k <= 64
    V = 3 + 2 * n
    parent = np.zeros(V, dtype=np.int64)
    parent[0] = -1
    parent[3:3 + n] = 1
    parent[3 + n:] = 2
    combos = np.arange(n)
    state = np.zeros((2, V), dtype=np.int64)
    for col, values in enumerate((combos // k, combos % k)):
        state[col, 3:3 + n] = values
        state[col, 3 + n:] = values[::-1]
    bins = (np.arange(V) >= 3).astype(np.int64)
    return parent, bins, one_hot_words(state, k)


@pytest.mark.parametrize('arity', [65, 'tile + 1'])
def test_order_independence_at_high_arity(arity):
    tile = sort_tile()
    assert tile >= 64
    n = tile + 1 if arity == 'tile + 1' else arity
    parent, bins, sets = two_stars(n, 64 if n > 1024 else 33)
    into, live, width, groups, info = device_pass(parent, bins, sets)
    assert into[2] == 1 and not live[2] and not live[3 + n:].any() and live[:2].all() and live[3:3 + n].all()
    assert width[1] == 2 and groups == 1 and info['levels'] == 3
    # one tip of one star in another state of column 0 (one that no tip has: nothing else becomes equal): the stars differ
    victim = 3 + n + n // 2
    sets[0, victim, 0] = np.uint64(1) << np.uint64(50)
    into, live, width, groups, info = device_pass(parent, bins, sets)
    assert into[2] == 2 and live.all() and groups == 0 and (width == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. depth: thousands of thin levels
def test_caterpillar_of_alternating_states():
    flat = caterpillar(2000)
    internal = flat.n_children > 0
    state = np.where(internal, flat.depth % 2, (flat.depth + 1) % 2)    # a tip takes the state of its parent
    sets = one_hot_words(state[None], 2)
    compressed = tc.compact(flat, *tc.collapse_host(flat, sets), columns=['c'], states=[np.array(['A', 'B'])], words=[sets[0]])
    assert compressed.n_vertices == 2000
    with hip.Engine.tree_only(flat) as eng:
        checked = CheckedEngine(eng)
        merged = tc.collapse_horizontally(compressed, engine=checked)
    assert checked.passes == 1 and merged.n_vertices == 2000 and merged.merged_groups == [0, 0]
    info = checked.infos[0]
    assert info['levels'] == 2000
    # one launch per level (a level here is one vertex with one child), the states, and the pass down: 2 + ceil(log2(levels)) + 1
    assert info['launches'] == 2000 + 1 + 2 + 11
    host = tc.collapse_horizontally(compressed, device=False)
    assert np.array_equal(merged.vertex, host.vertex) and np.array_equal(merged.width, host.width)


# ---------------------------------------------------------------------------------------------------------------------
# 4. many equal and near-equal configurations in the table at once (the table at its normal size)
@pytest.mark.parametrize('n_cols', [1, 3, 33])
def test_collision_pressure(n_cols):
    rng = np.random.default_rng(n_cols)
    V = 5000
    parent = np.zeros(V, dtype=np.int64)
    parent[0] = -1
    ids = np.arange(1, V)
    near = ids - 1 - rng.integers(0, 6, size=V - 1)
    parent[1:] = np.where((rng.random(V - 1) < 0.15) | (near < 1), 0, near)      # small random trees under one root
    state = np.zeros((n_cols, V), dtype=np.int64)
    flip = rng.random(V) < 0.3                                                   # ... most vertices alike, the others one column off
    state[rng.integers(0, n_cols, size=V)[flip], np.flatnonzero(flip)] = 1
    sets = one_hot_words(state, 2)
    bins = rng.integers(0, 2, size=V)
    into, live, width, groups, info = device_pass(parent, bins, sets)
    assert groups > 100 and 100 < live.sum() < V and width.max() > 2
    assert info['table_slots'] >= 2 * (V * (2 * n_cols + 2) + 2 * (V - 1))     # twice the pairs a pass can make


# ---------------------------------------------------------------------------------------------------------------------
# 5. widths of a set
@pytest.mark.parametrize('k', [64, 65, 512])
def test_difference_in_the_last_word_of_the_last_column(k):
    W = (k + 63) // 64
    parent = np.array([-1, 0, 0, 0])
    sets = np.zeros((2, 4, W), dtype=np.uint64)
    sets[:, :, 0] = 1
    sets[1, 1:, W - 1] |= np.uint64(1) << np.uint64((k - 1) % 64)
    into, live, width, groups, _ = device_pass(parent, np.zeros(4, int), sets)
    assert into.tolist() == [0, 1, 1, 1] and width.tolist() == [1, 3, 1, 1] and groups == 1
    sets[1, 3, W - 1] ^= np.uint64(1) << np.uint64((k - 1) % 64)
    into, live, width, groups, _ = device_pass(parent, np.zeros(4, int), sets)
    assert into.tolist() == [0, 1, 1, 3] and live.tolist() == [True, True, False, True] and width.tolist() == [1, 2, 1, 1]


def test_wider_sets_are_refused_or_go_to_the_host():
    flat = FlatForest.balanced(3)
    words = np.ones((flat.n_nodes, 9), dtype=np.uint64)
    words[flat.n_children == 0, 8] = 2
    sets = words[None]
    compressed = tc.compact(flat, *tc.collapse_host(flat, sets), columns=['c'], states=[np.arange(576)], words=[words])
    with pytest.raises(ValueError, match='9 words'):
        tc.collapse_horizontally(compressed, device=True)
    merged = tc.collapse_horizontally(compressed, device=None)      # numpy, whatever devices there are
    host = tc.collapse_horizontally(compressed, device=False)
    assert np.array_equal(merged.vertex, host.vertex) and np.array_equal(merged.width, host.width)
    assert merged.n_vertices == 2 and merged.width.tolist() == [1, 8]
    with hip.Engine.tree_only(flat) as eng:
        with pytest.raises(hip.HipError):
            eng.compress_horizontal(compressed.parent, compressed.order, np.zeros(9, int), np.ones(9, int), np.ones(9, bool),
                                    tc.stacked_sets(compressed.words, 9))


# ---------------------------------------------------------------------------------------------------------------------
# 6. the smallest forests
def test_degenerate_forests():
    one = np.ones((1, 1, 1), dtype=np.uint64)
    into, live, width, groups, info = device_pass(np.array([-1]), np.array([1]), one)
    assert (into.tolist(), live.tolist(), width.tolist(), groups, info['levels']) == ([0], [True], [1], 0, 1)
    # single nodes: roots never merge, however equal
    into, live, width, groups, info = device_pass(np.full(3, -1), np.ones(3, int), np.ones((1, 3, 1), dtype=np.uint64))
    assert into.tolist() == [0, 1, 2] and live.all() and (width == 1).all() and groups == 0 and info['levels'] == 1
    # nothing to merge
    sets = np.array([[[1], [1], [2]]], dtype=np.uint64)
    into, live, width, groups, info = device_pass(np.array([-1, 0, 0]), np.ones(3, int), sets)
    assert into.tolist() == [0, 1, 2] and live.all() and (width == 1).all() and groups == 0 and info['levels'] == 2
    # no live vertex at all: nothing is launched
    into, live, width, groups, info = device_pass(np.array([-1, 0]), np.ones(2, int), np.ones((1, 2, 1), dtype=np.uint64),
                                                  live=np.zeros(2, dtype=bool))
    assert into.tolist() == [0, 1] and not live.any() and info['launches'] == 0 and info['levels'] == 0


def test_bad_vertex_forests_are_errors():
    sets = np.ones((1, 3, 1), dtype=np.uint64)
    with hip.Engine.tree_only(FlatForest.balanced(2)) as eng:
        for parent, bins, width in (([-1, 0, 7], [0, 0, 0], [1, 1, 1]), ([-1, 2, 1], [0, 0, 0], [1, 1, 1]),
                                    ([-1, 0, 0], [0, -1, 0], [1, 1, 1]), ([-1, 0, 0], [0, 0, 0], [1, 0, 1])):
            with pytest.raises(hip.HipError):
                eng.compress_horizontal(parent, np.arange(3), bins, width, np.ones(3, bool), sets)
        with pytest.raises(ValueError):
            eng.compress_horizontal([-1, 0, 0], np.arange(2), [0, 0, 0], [1, 1, 1], np.ones(3, bool), sets)


# ---------------------------------------------------------------------------------------------------------------------
# 7. on a context that is busy with something else
def test_on_a_context_with_columns_and_a_sweep():
    flat = synthetic.balanced_forest(6)
    k = 4
    states = synthetic.tip_states(flat.n_tips, k, 0)
    spec = dict(kind=0, pi=synthetic.f81_frequencies(k, 0))
    case_flat, columns, column2states, expected = load_case('two_passes')
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([(spec, (1.0, 0.0, 1.0))])
        eng.set_tip_states(states)
        lnl = np.array(eng.bottom_up(True))
        eng.top_down_marginals()
        before = [eng.download(what).copy() for what in (hip.BUF_BU, hip.BUF_TD, hip.BUF_POSTERIOR)]
        held = eng.memory()
        compressed = tc.collapse_vertically(case_flat, columns, column2states, device=False)
        checked = CheckedEngine(eng)
        merged = tc.collapse_horizontally(compressed, engine=checked)
        assert checked.passes == 2 and eng.memory()[0] == held[0]
        for what, kept in zip((hip.BUF_BU, hip.BUF_TD, hip.BUF_POSTERIOR), before):
            assert np.array_equal(eng.download(what), kept)
        assert np.isfinite(lnl).all()
    assert tc.pajek_lines(merged, columns)[0] == [str(v) for v in expected['vertices']]
