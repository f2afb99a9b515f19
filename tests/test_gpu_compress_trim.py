"""
The trimming on the device (pml_compress_trim, pastml_amd.visualisation.tree_compressor) against the reference's lines
(tests/golden/compress_trim.npz) and, on built inputs, against the host restatement -- which test_compress_trim_host.py pins to
the same goldens.  Every device call in this file is compared with ``trim_host`` array for array, dtype and values (NaN
thresholds equal NaN).  Integer and exactly rounded float64 work: every comparison is exact.
"""
import numpy as np
import pytest

from pastml_amd import hip, synthetic
from pastml_amd.tree import FlatForest
from pastml_amd.visualisation import tree_compressor as tc
from test_compress_trim_host import CASES, check_against_golden, load_case

pytestmark = pytest.mark.gpu

NAMES = ('tsize', 'keep', 'spliced', 'new_parent', 'moved', 'threshold')


class CheckedEngine(object):
    """An engine whose every trimming call and horizontal pass is compared with the host restatement."""

    def __init__(self, engine):
        self.engine = engine
        self.trims = 0
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
        return device

    def compress_trim(self, *args):
        device = self.engine.compress_trim(*args)
        host = tc.trim_host(*args)
        for name, d, h in zip(NAMES, device, host):
            assert d.dtype == h.dtype and d.shape == h.shape and np.array_equal(d, h, equal_nan=d.dtype == np.float64), name
        self.trims += 1
        self.infos.append(self.engine.compress_trim_info())
        return device


@pytest.fixture(scope='module')
def engine():
    """(the context supplies the device and the stream, no more)"""
    with hip.Engine.tree_only(FlatForest.balanced(2)) as eng:
        yield eng


def device_trim(engine, parent, T, sets, k, w=None, tree=None, trim_tree=(True,)):
    """One call on arrays, compared with the host: dict of the outputs and ``info``."""
    L = len(parent)
    checked = CheckedEngine(engine)
    out = checked.compress_trim(np.asarray(parent), np.zeros(L, int) if tree is None else tree, np.asarray(T),
                                np.ones(L, int) if w is None else w, sets, k, np.asarray(trim_tree, dtype=bool))
    result = dict(zip(NAMES, out))
    result['info'] = checked.infos[0]
    return result


def distinct_sets(L):
    return np.arange(1, L + 1, dtype=np.uint64).reshape(1, L, 1)


def launches_of(levels, trimmed=True):
    return tc.jump_rounds(levels) + (9 if trimmed else 3)


# ---------------------------------------------------------------------------------------------------------------------
# 1. device = reference
@pytest.mark.parametrize('case', CASES)
def test_device_reproduces_the_reference(case, tmp_path):
    flat, columns, column2states, expected = load_case(case)
    k, can_merge = int(expected['tip_size_threshold']), bool(expected['can_merge'])
    with hip.Engine.tree_only(flat) as eng:
        checked = CheckedEngine(eng)
        trimmed = tc.compress_tree(flat, columns, column2states, tip_size_threshold=k, can_merge_diff_sizes=can_merge, engine=checked)
    assert checked.trims == 1
    check_against_golden(trimmed, columns, expected, tmp_path)
    host = tc.compress_tree(flat, columns, column2states, tip_size_threshold=k, can_merge_diff_sizes=can_merge, device=False)
    for field in ('vertex', 'width', 'parent', 'members', 'member_offsets', 'n_tips_total', 'removed', 'mediators'):
        assert np.array_equal(getattr(trimmed, field), getattr(host, field)), field
    assert trimmed.merged_groups == host.merged_groups
    # ... and with a context of the module's own making
    own = tc.compress_tree(flat, columns, column2states, tip_size_threshold=k, can_merge_diff_sizes=can_merge, device=True)
    assert tc.pajek_lines(own, columns) == tc.pajek_lines(host, columns)


# ---------------------------------------------------------------------------------------------------------------------
# 2. depth: a path of vertices
def path(n, big_at):
    """A path of n vertices whose tips alternate 2, 1, 2, ... (so that every second vertex is a candidate), 100 at ``big_at``."""
    T = np.where(np.arange(n) % 2 == 1, 2, 1)
    T[0] = 0
    T[big_at] = 100
    return np.arange(-1, n - 1), T, distinct_sets(n)


def test_caterpillar(engine):
    n = 2000
    parent, T, sets = path(n, n - 1)
    deep = device_trim(engine, parent, T, sets, 1)
    assert deep['threshold'][0] == 100 and deep['keep'].all() and not deep['spliced'].any()   # all of them lead to the big tip
    assert deep['info']['levels'] == n and deep['info']['rounds'] == 11 and deep['info']['launches'] == launches_of(n)
    parent, T, sets = path(n, 1)
    top = device_trim(engine, parent, T, sets, 1)
    assert top['threshold'][0] == 100 and top['keep'].tolist() == [True, True] + [False] * (n - 2)   # the cascade from the bottom
    short = device_trim(engine, *path(20, 19), 1)
    assert short['keep'].all() and short['info']['rounds'] == 5 and short['info']['launches'] == launches_of(20)


# ---------------------------------------------------------------------------------------------------------------------
# 3. chains of mediators
def chain(m, failing=None):
    """Root {A}; m candidates {A, B} one under the other; c {B} with 5 tips; root's other children of 4 tips and of 1."""
    L = m + 4
    parent = np.concatenate(([-1], np.arange(m + 1), [0, 0]))
    T = np.zeros(L, dtype=int)
    T[m + 1:] = (5, 4, 1)
    sets = np.full((1, L, 1), 3, dtype=np.uint64)
    sets[0, 0], sets[0, m + 1:, 0] = 1, (2, 4, 8)
    if failing is not None:
        sets[0, failing] = 2   # {B} alone: it stays, the one under it no longer has {A, B} above it, those above it see {B} below
    return parent, T, sets


@pytest.mark.parametrize('m', [1, 2, 65, 300])
def test_mediator_chains(engine, m):
    out = device_trim(engine, *chain(m), 2)
    assert out['threshold'][0] == 4 and out['keep'].tolist() == [True] * (m + 3) + [False]
    assert out['spliced'].tolist() == [False] + [True] * m + [False] * 3
    assert out['new_parent'][m + 1] == 0 and out['moved'].tolist() == [False] * (m + 1) + [True, False, False]
    assert out['info']['launches'] == launches_of(m + 2)          # one launch for the chains, however long
    mid = 1 + m // 2
    out = device_trim(engine, *chain(m, failing=mid), 2)
    assert out['spliced'].tolist() == [i not in (mid, mid + 1) and 1 <= i <= m for i in range(m + 4)]
    assert out['new_parent'][mid] == 0 and out['new_parent'][m + 1] == min(mid + 1, m) and out['moved'][mid] == (mid != 1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the prefix count across workgroups
@pytest.mark.parametrize('big_at', ['last', 'first'])
def test_star_across_tiles(engine, big_at):
    """Root, a hub under it, 5 000 leaves under the hub: the hub's run spans every tile of the scan."""
    n = 5000
    L = n + 3
    parent = np.concatenate(([-1, 0], np.full(n, 1), [0]))
    T = np.concatenate(([0, 0], np.ones(n, int), [1]))
    big = L - 2 if big_at == 'last' else 2
    T[big] = 10
    out = device_trim(engine, parent, T, distinct_sets(L), 1)
    assert out['info']['scan_tile'] * 2 < L and out['threshold'][0] == 10
    assert np.flatnonzero(out['keep']).tolist() == [0, 1, big]


def random_preorder(L, rng):
    parent = np.full(L, -1, dtype=np.int64)
    path_ = [0]
    for i in range(1, L):
        up = int(rng.integers(max(0, len(path_) - 3), len(path_)))    # hang it under one of the last few of the rightmost path
        del path_[up + 1:]
        parent[i] = path_[-1]
        path_.append(i)
    return parent


@pytest.mark.parametrize('size', ['tile', 'tile - 1', 'tile + 1', '2 * tile + 1'])
def test_sizes_around_the_scan_tile(engine, size):
    tile = engine.compress_trim_info()['scan_tile']
    assert tile >= 64
    L = eval(size, dict(tile=tile))
    rng = np.random.default_rng(L)
    parent = random_preorder(L, rng)
    has_child = np.zeros(L, dtype=bool)
    has_child[parent[1:]] = True
    T = np.where(has_child, rng.integers(0, 2, L) * rng.integers(0, 3, L), rng.integers(1, 40, L))
    w = np.where(np.arange(L) == 0, 1, rng.choice([1, 1, 1, 2, 3], L))
    sets = rng.integers(1, 8, size=(2, L, 1)).astype(np.uint64)
    out = device_trim(engine, parent, T, sets, 25, w=w)
    assert not np.isnan(out['threshold'][0]) and 25 <= out['keep'].sum() < L and out['info']['launches'] == \
        launches_of(out['info']['levels'])
    # the last entry alone is big: the count has to reach it
    T[:] = np.where(has_child, 0, 1)
    T[L - 1] = 7
    out = device_trim(engine, parent, T, sets, 1)
    assert out['threshold'][0] == 7 and out['keep'][L - 1] and not out['keep'][~has_child][:-1].any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. widths of a set
@pytest.mark.parametrize('k', [64, 65, 512])
def test_deciding_bit_in_the_last_word_of_the_last_column(engine, k):
    W = (k + 63) // 64
    last = np.uint64(1) << np.uint64((k - 1) % 64)
    parent = np.array([-1, 0, 1, 0, 0])
    T = np.array([0, 0, 5, 4, 1])
    sets = np.zeros((2, 5, W), dtype=np.uint64)
    sets[0, :, 0] = (1, 3, 2, 4, 8)               # column 0: root {A}, n {A, B}, c {B}
    sets[1, 0, 0] = 1
    sets[1, 1, 0], sets[1, 1, W - 1] = 1, sets[1, 1, W - 1] | last   # column 1: n = root's state and state k - 1 ...
    sets[1, 1, 0] |= 1
    sets[1, 2, W - 1] = last                                          # ... which is c's
    sets[1, 3:, 0] = 1
    out = device_trim(engine, parent, T, sets, 2)
    assert out['spliced'].tolist() == [False, True, False, False, False] and out['new_parent'].tolist() == [-1, -1, 0, 0, -1]
    sets[1, 2, W - 1] = last >> np.uint64(1)                          # c in the state next to it: n is no mediator
    out = device_trim(engine, parent, T, sets, 2)
    assert not out['spliced'].any() and out['new_parent'].tolist() == [-1, 0, 1, 0, -1]


def test_wider_sets_are_refused_or_go_to_the_host(engine):
    flat = FlatForest.balanced(3)
    words = np.ones((flat.n_nodes, 9), dtype=np.uint64)
    words[flat.n_children == 0, 8] = 2 + np.arange(8, dtype=np.uint64)
    compressed = tc.compact(flat, *tc.collapse_host(flat, words[None]), columns=['c'], states=[np.arange(576)], words=[words])
    merged = tc.collapse_horizontally(compressed, tip_size_threshold=3, device=False)
    assert merged.n_vertices == 9
    with pytest.raises(ValueError, match='9 words'):
        tc.trim(merged, tip_size_threshold=3, device=True)
    trimmed = tc.trim(merged, tip_size_threshold=3, device=None)      # numpy, whatever devices there are
    host = tc.trim(merged, tip_size_threshold=3, device=False)
    assert np.array_equal(trimmed.vertex, host.vertex) and np.isnan(trimmed.threshold).all()
    with pytest.raises(hip.HipError):
        engine.compress_trim(merged.parent, np.zeros(9, int), merged.n_tips_total, merged.width,
                             tc.stacked_sets([words[merged.vertex]], 9), 3, [True])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the smallest forests
def test_degenerate_forests(engine):
    one = device_trim(engine, [-1], [1], distinct_sets(1), 0)
    assert one['keep'].tolist() == [True] and np.isnan(one['threshold'][0]) and one['info']['launches'] == launches_of(1, False)
    # no tree over the gate: nothing is launched
    parent, T = np.array([-1, 0, 0, -1, 3]), np.array([0, 1, 5, 0, 2])
    none = device_trim(engine, parent, T, distinct_sets(5), 1, tree=np.array([0, 0, 0, 1, 1]), trim_tree=[False, False])
    assert none['info']['launches'] == 0 and none['keep'].all() and (none['tsize'] == 0).all() and np.isnan(none['threshold']).all()
    assert none['new_parent'].tolist() == parent.tolist()
    # all candidates tied: the smallest is the threshold, nothing happens, nothing more is launched
    tied = device_trim(engine, [-1, 0, 0, 0], [0, 3, 3, 3], distinct_sets(4), 2)
    assert np.isnan(tied['threshold'][0]) and tied['keep'].all() and tied['tsize'].tolist() == [0, 3, 3, 3]
    assert tied['info']['launches'] == launches_of(2, False)
    # the second tree alone
    second = device_trim(engine, parent, T, distinct_sets(5), 1, tree=np.array([0, 0, 0, 1, 1]), trim_tree=[False, True])
    assert second['tsize'].tolist() == [0, 0, 0, 0, 2] and np.isnan(second['threshold']).all()


def test_bad_vertex_forests_are_errors(engine):
    sets = distinct_sets(4)
    good = dict(parent=[-1, 0, 1, 0], T=[0, 0, 2, 1], w=[1, 1, 1, 1])
    for bad in (dict(parent=[-1, 2, 1, 0]), dict(parent=[-1, 1, 1, 0]), dict(parent=[-1, 0, 0, 1]), dict(w=[1, 0, 1, 1]),
                dict(T=[0, 0, -2, 1])):
        args = dict(good)
        args.update(bad)
        with pytest.raises(hip.HipError):
            engine.compress_trim(args['parent'], np.zeros(4, int), args['T'], args['w'], sets, 1, [True])
        with pytest.raises(ValueError):
            tc.trim_host(args['parent'], np.zeros(4, int), args['T'], args['w'], sets, 1, [True])
    with pytest.raises(hip.HipError):   # widths of 2^20 down a path of three
        engine.compress_trim([-1, 0, 1, 2, 0], np.zeros(5, int), [0, 0, 0, 1, 2], [1, 2 ** 20, 2 ** 20, 2 ** 20, 1],
                             distinct_sets(5), 1, [True])
    with pytest.raises(ValueError):
        engine.compress_trim([-1, 0, 0], np.zeros(2, int), [0, 1, 1], [1, 1, 1], distinct_sets(3), 1, [True])
    ok = device_trim(engine, good['parent'], good['T'], sets, 1)    # the context is as good as before
    assert ok['threshold'][0] == 2 and ok['keep'].tolist() == [True, True, True, False]


# ---------------------------------------------------------------------------------------------------------------------
# 7. on a context that is busy with something else
def test_on_a_context_with_columns_and_a_sweep():
    flat = synthetic.balanced_forest(6)
    k = 4
    states = synthetic.tip_states(flat.n_tips, k, 0)
    spec = dict(kind=0, pi=synthetic.f81_frequencies(k, 0))
    case_flat, columns, column2states, expected = load_case('ragged')
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([(spec, (1.0, 0.0, 1.0))])
        eng.set_tip_states(states)
        lnl = np.array(eng.bottom_up(True))
        eng.top_down_marginals()
        before = [eng.download(what).copy() for what in (hip.BUF_BU, hip.BUF_TD, hip.BUF_POSTERIOR)]
        held = eng.memory()
        merged = tc.compress_forest(case_flat, columns, column2states, timing=tc.HORIZONTAL,
                                    tip_size_threshold=int(expected['tip_size_threshold']), device=False)
        checked = CheckedEngine(eng)
        trimmed = tc.trim(merged, tip_size_threshold=int(expected['tip_size_threshold']), engine=checked)
        assert checked.trims == 1 and checked.passes == 1 and eng.memory()[0] == held[0]
        for what, kept in zip((hip.BUF_BU, hip.BUF_TD, hip.BUF_POSTERIOR), before):
            assert np.array_equal(eng.download(what), kept)
        assert np.isfinite(lnl).all()
    assert tc.pajek_lines(trimmed, columns)[0] == [str(v) for v in expected['vertices']]
