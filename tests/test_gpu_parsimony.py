"""
The parsimony passes on the device (pml_parsimony, pastml_amd.parsimony.parsimonious_acr_batch) against the reference's
pastml/parsimony.py (tests/golden/parsimony.npz, parsimony_wide.npz) and, at sizes the reference cannot reach in a test,
against the host path -- unchanged code that the goldens pin to the reference.  Integer work: every comparison is exact.
The counter widths (arities around 14 / 15, 254 / 255, 65534 / 65535), every lane group W = 1 .. 8, ties across words, unary
nodes, lone tips and stars: tests/test_gpu_parsimony_shapes.py, on the cases of tests/parsimony_shape_cases.py (host side:
tests/test_parsimony_shape_cases_host.py, which also pins the host path to the reference on those forests).
"""
import os

import numpy as np
import pytest

from conftest import load_golden, GOLDEN
from pastml_amd import hip
from pastml_amd import parsimony as P
from pastml_amd.batch import masks_from_words
from pastml_amd.parsimony import STEPS, MP, DOWNPASS, ACCTRAN, DELTRAN
from pastml_amd.tree import FlatForest, get_flat_forest

pytestmark = pytest.mark.gpu
ALL_METHODS = hip.PARS_ACCTRAN | hip.PARS_DOWNPASS | hip.PARS_DELTRAN


def random_given(flat, k, n_cols, seed):
    """Packed annotations [n_cols, N, W]: 10 % of the tips none, 10 % three states, the others one; 3 % of the internal nodes one."""
    rng = np.random.default_rng(seed)
    N = flat.n_nodes
    tips = np.asarray(flat.n_children) == 0
    ann = np.zeros((n_cols, N, k), dtype=np.int8)
    u = rng.random((n_cols, N))
    one = rng.integers(k, size=(n_cols, N))
    keep = np.where(tips, u >= 0.1, u < 0.03)
    c, n = np.nonzero(keep)
    ann[c, n, one[c, n]] = 1
    c, n = np.nonzero(tips & (u >= 0.1) & (u < 0.2))
    for _ in range(2):
        ann[c, n, rng.integers(k, size=len(c))] = 1
    return hip.pack_masks(ann, k)


def host_passes(flat, given, k):
    """(sets int32 [3, N, k], steps [3], sizes histogram [3, k + 1]) of one character by the host path: ACCTRAN, DOWNPASS, DELTRAN."""
    g = masks_from_words(given, k).astype(np.int32)
    initial = np.where(g.any(axis=1, keepdims=True), g, 1).astype(np.int32)
    bu = P.uppass(flat, initial)
    down = P.downpass(flat, bu, initial)
    sets = [P.acctran(flat, bu), down, P.deltran(flat, down)]
    steps = [P.num_parsimonious_steps(flat, s) for s in sets]
    hist = [np.bincount(s.sum(axis=1), minlength=k + 1) for s in sets]
    return np.stack(sets), np.array(steps), np.stack(hist)


def assert_device_equals_host(flat, k, n_cols, seed, tune=None, check_cols=None):
    given = random_given(flat, k, n_cols, seed)
    with hip.Engine.tree_only(flat, tune=tune) as eng:
        sets, steps, hist = eng.parsimony(given, k, ALL_METHODS)
    for c in (range(n_cols) if check_cols is None else check_cols):
        hs, hsteps, hhist = host_passes(flat, given[c], k)
        for j in range(3):
            assert np.array_equal(masks_from_words(sets[j, c], k), hs[j]), (c, j)
        assert steps[:, c].tolist() == hsteps.tolist(), c
        assert np.array_equal(hist[:, c], hhist), c
    return given, sets, steps, hist


def caterpillar(depth):
    """Root, then per depth an internal node and a tip; two tips at the bottom.  Level order ids."""
    N = 2 * depth + 1
    ids = np.arange(N)
    d = (ids + 1) // 2                      # depth of node i
    parent = np.where(d <= 1, 0, 2 * (d - 1) - 1).astype(np.int32)
    parent[0] = -1
    internal = (ids == 0) | ((ids % 2 == 1) & (d < depth))
    n_children = np.where(internal, 2, 0).astype(np.int32)
    first_child = np.where(ids == 0, 1, 2 * d + 1).astype(np.int32)
    return FlatForest(parent, n_children, first_child, np.full(N, 0.1), np.array([0]))


def star(n_tips):
    N = n_tips + 1
    parent = np.zeros(N, dtype=np.int32)
    parent[0] = -1
    n_children = np.zeros(N, dtype=np.int32)
    n_children[0] = n_tips
    return FlatForest(parent, n_children, np.full(N, 1, dtype=np.int32), np.full(N, 0.1), np.array([0]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. device = reference
def forest_of(z, prefix):
    flat = FlatForest(z[prefix + 'parent'], z[prefix + 'n_children'], z[prefix + 'first_child'], z[prefix + 'dist'],
                      np.arange(int(z[prefix + 'n_roots'])))
    return flat, flat.to_tree_nodes(names=list(z[prefix + 'node_names']))


@pytest.mark.parametrize('prefix,character', [('alb_', 'Country'), ('poly_', 'ch'), ('forest_', 'ch')])
def test_device_matches_reference(prefix, character):
    z = load_golden('parsimony')
    states, ann = z[prefix + 'states'], z[prefix + 'annotation']
    s2i = {s: i for i, s in enumerate(states)}
    for method in (MP, DOWNPASS, ACCTRAN, DELTRAN):
        flat, roots = forest_of(z, prefix)
        for i, n in enumerate(flat.nodes):
            if ann[i].any():
                n.add_feature(character, set(states[ann[i].astype(bool)]))
        results, = P.parsimonious_acr_batch(roots, [character], [method], [states], flat.n_nodes, flat.n_tips)
        assert [r['method'] for r in results] == [m for m in (ACCTRAN, DOWNPASS, DELTRAN) if method in (MP, m)]
        for res in results:
            tag = '{}{}_{}_'.format(prefix, method, res['method'])
            assert res['character'] == str(z[tag + 'character'])
            sel = np.zeros_like(ann)
            for i, n in enumerate(flat.nodes):
                for s in getattr(n, res['character']):
                    sel[i, s2i[s]] = 1
            assert np.array_equal(sel, z[tag + 'selected']), tag
            assert res[STEPS] == int(z[tag + 'steps']), tag
            assert float(res['num_scenarios']) == float(z[tag + 'num_scenarios'])
            assert res['num_unresolved_nodes'] == int(z[tag + 'num_unresolved_nodes'])
            assert res['num_states_per_node_avg'] == float(z[tag + 'num_states_per_node_avg'])
            assert res['num_nodes'] == flat.n_nodes and res['num_tips'] == flat.n_tips


@pytest.mark.parametrize('prefix', ['a_', 'b_', 'c_'])
def test_device_matches_reference_wide(prefix):
    z = load_golden('parsimony_wide')
    n_tips, seed, max_arity, n_trees = (int(v) for v in z[prefix + 'spec'])
    flat = FlatForest.random(n_tips, seed=seed, max_arity=max_arity, zero_frac=float(z[prefix + 'zero_frac']), n_trees=n_trees)
    assert np.array_equal(np.asarray(flat.parent), z[prefix + 'parent'])
    roots = [flat.nodes[r] for r in flat.roots]
    states = z[prefix + 'states']
    k = len(states)
    ann = masks_from_words(z[prefix + 'annotation'], k).astype(bool)
    for method in (MP, DOWNPASS, ACCTRAN, DELTRAN):
        for i, n in enumerate(flat.nodes):
            if ann[i].any():
                n.add_feature('ch', set(states[ann[i]]))
            else:
                n.del_feature('ch')
        results, = P.parsimonious_acr_batch(roots, ['ch'], [method], [states], flat.n_nodes, flat.n_tips)
        tag = prefix + method + '_'
        assert [r['method'] for r in results] == list(z[tag + 'methods'])
        assert [r['character'] for r in results] == list(z[tag + 'characters'])
        assert [r[STEPS] for r in results] == z[tag + 'steps'].tolist()
        assert [str(r['num_scenarios']) for r in results] == list(z[tag + 'num_scenarios'])
        assert [r['num_unresolved_nodes'] for r in results] == z[tag + 'num_unresolved_nodes'].tolist()
        assert [r['num_states_per_node_avg'] for r in results] == z[tag + 'num_states_per_node_avg'].tolist()
        columns = get_flat_forest(roots).columns   # (node ids: forest-wide level order, as in the fixture)
        for r in results:
            assert np.array_equal(columns[r['character']].words, z[prefix + r['method'] + '_selected']), (tag, r['method'])


# ---------------------------------------------------------------------------------------------------------------------
# 2. device = host path at sizes beyond the reference's reach
def test_large_binary_tree_k64():
    assert_device_equals_host(FlatForest.random(262144, seed=1), 64, 4, seed=2)


def test_forest_with_polytomies_k20():
    assert_device_equals_host(FlatForest.random(100000, seed=3, max_arity=5), 20, 16, seed=4, check_cols=(0, 7, 15))


def test_caterpillar():
    assert_device_equals_host(caterpillar(10000), 4, 2, seed=5)


def test_star_of_5000_tips():
    assert_device_equals_host(star(5000), 6, 3, seed=6)


@pytest.mark.parametrize('k', [1, 64, 65, 512])
def test_state_counts_at_the_word_boundaries(k):
    assert_device_equals_host(FlatForest.random(3000, seed=7 + k, max_arity=4, n_trees=2), k, 3, seed=8)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the library's numbering is invisible
def test_numbering_is_invisible():
    flat = FlatForest.random(40000, seed=9, max_arity=3)
    k = 70
    given = random_given(flat, k, 3, seed=10)
    outs = []
    for tune in (None, dict(NO_HEIGHT_ORDER=1), dict(SHAPE_ORDER=1)):
        with hip.Engine.tree_only(flat, tune=tune) as eng:
            outs.append(eng.parsimony(given, k, ALL_METHODS))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)
    hs, hsteps, hhist = host_passes(flat, given[1], k)
    assert np.array_equal(masks_from_words(outs[0][0][:, 1], k), hs)
    assert outs[0][1][:, 1].tolist() == hsteps.tolist() and np.array_equal(outs[0][2][:, 1], hhist)


# ---------------------------------------------------------------------------------------------------------------------
# 4. columns are independent, and so is the entry's own chunking
def test_columns_are_independent():
    flat = FlatForest.random(5000, seed=11, max_arity=4)
    k = 12
    given = random_given(flat, k, 32, seed=12)
    one = given[5:6]
    first = np.concatenate([one, given[:31]])
    last = np.concatenate([given[:31], one])
    with hip.Engine.tree_only(flat) as eng:
        alone = eng.parsimony(one, k, ALL_METHODS)
        as_first = eng.parsimony(first, k, ALL_METHODS)
        as_last = eng.parsimony(last, k, ALL_METHODS)
        whole = eng.parsimony(given, k, ALL_METHODS)
    with hip.Engine.tree_only(flat, tune=dict(PARS_MAX_COLS=5)) as eng:   # 32 columns in chunks of 5, 5, ..., 2
        chunked = eng.parsimony(given, k, ALL_METHODS)
    for a, f, l in zip(alone, as_first, as_last):
        assert np.array_equal(a[:, 0], f[:, 0]) and np.array_equal(a[:, 0], l[:, 31])
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)
    # a subset of the methods gives the same sets in the slots it fills
    with hip.Engine.tree_only(flat) as eng:
        sets, steps, hist = eng.parsimony(given[:2], k, hip.PARS_DELTRAN)
    assert np.array_equal(sets[0], whole[0][2, :2]) and np.array_equal(steps[0], whole[1][2, :2])
    assert np.array_equal(hist[0], whole[2][2, :2])


# ---------------------------------------------------------------------------------------------------------------------
# 5. acr()
def _acr_inputs():
    import pandas as pd
    flat = FlatForest.random(700, seed=13, max_arity=5, zero_frac=0.05, n_trees=2)
    rng = np.random.default_rng(14)
    tips = [n for n in flat.nodes if n.is_leaf()]
    table = {}
    for name, k in (('a', 3), ('b', 5), ('c', 3), ('d', 7), ('e', 4), ('f', 4)):
        values = np.array(['{}{}'.format(name, i) for i in range(k)], dtype=object)[rng.integers(k, size=len(tips))]
        values[rng.random(len(tips)) < 0.1] = None
        table[name] = values
    return flat, pd.DataFrame(table, index=[n.name for n in tips])


def _run_acr(monkeypatch, path, methods, **kwargs):
    from pastml_amd.acr import acr
    monkeypatch.setenv(P.PATH_VARIABLE, path)
    np.random.seed(0)   # (acr() draws the optimisers' restart seeds)
    flat, df = _acr_inputs()
    roots = [flat.nodes[r] for r in flat.roots]
    results = acr(roots, df, prediction_method=methods, **kwargs)
    features = {r['character']: [getattr(n, r['character'], None) for n in flat.nodes] for r in results}
    return results, features


def _assert_same_results(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert sorted(ra) == sorted(rb)
        for key in ra:
            if key == 'states':
                assert list(ra[key]) == list(rb[key])
            elif key == 'model':
                continue
            elif isinstance(ra[key], float):
                assert ra[key] == pytest.approx(rb[key], rel=1e-9), key
            elif hasattr(ra[key], 'values'):
                np.testing.assert_allclose(ra[key].values, rb[key].values, rtol=1e-9)
            else:
                assert ra[key] == rb[key], key


@pytest.mark.parametrize('methods', [MP, DOWNPASS, ACCTRAN, DELTRAN, [MP, 'COPY', 'MPPA', DELTRAN, ACCTRAN, DOWNPASS]])
def test_acr_device_equals_host(monkeypatch, methods):
    device, device_features = _run_acr(monkeypatch, 'device', methods)
    host, host_features = _run_acr(monkeypatch, 'host', methods)
    _assert_same_results(device, host)
    assert device_features == host_features
    for r in device:
        if r['method'] in (ACCTRAN, DOWNPASS, DELTRAN):
            assert isinstance(r['num_scenarios'], int) and STEPS in r


def test_acr_mp_is_one_device_call(monkeypatch):
    calls = []
    real = hip.Engine.parsimony

    def counted(self, given, k, methods):
        calls.append((np.asarray(given).shape[0], k))
        return real(self, given, k, methods)

    monkeypatch.setattr(hip.Engine, 'parsimony', counted)
    monkeypatch.setenv(P.PATH_VARIABLE, 'device')
    from pastml_amd.acr import acr
    import pandas as pd
    flat = FlatForest.random(500, seed=15)
    tips = [n for n in flat.nodes if n.is_leaf()]
    rng = np.random.default_rng(16)
    df = pd.DataFrame({'c{}'.format(j): np.array(['x', 'y', 'z'], dtype=object)[rng.integers(3, size=len(tips))] for j in range(9)},
                      index=[n.name for n in tips])
    res = acr([flat.nodes[0]], df, prediction_method=MP)
    assert len(res) == 27 and calls == [(9, 3)]


def test_all_meta_method_on_the_device(monkeypatch):
    """What tests/test_parsimony.py::test_all_meta_method_matches_reference checks, with the parsimonious reconstructions
    of ALL computed on the device (on the group's own context)."""
    import pandas as pd
    from pastml_amd.acr import acr
    from pastml_amd.tree import read_tree
    monkeypatch.setenv(P.PATH_VARIABLE, 'device')
    calls = []
    real = hip.Engine.parsimony
    monkeypatch.setattr(hip.Engine, 'parsimony', lambda self, *a: (calls.append(self.n_cols), real(self, *a))[1])
    z = load_golden('parsimony')
    tree = read_tree(os.path.join(GOLDEN, 'data', 'Albanian.tree.152tax.tre'))
    df = pd.read_csv(os.path.join(GOLDEN, 'data', 'data.txt'), index_col=0, header=0)[['Country']]
    res = acr(tree, df, prediction_method='ALL', model='F81')
    assert calls == [1]   # one call, on the batch's context (it has the character's column)
    assert [r['method'] for r in res] == list(z['all_methods'])
    assert [r['character'] for r in res] == list(z['all_characters'])
    last = res[-1]
    assert sorted(last.keys()) == list(z['all_mppa_keys'])
    for key in z.files:
        if key.startswith('all_log_likelihood'):
            np.testing.assert_allclose(last[key[4:]], float(z[key]), rtol=1e-6, err_msg=key)
    for r in res[2:5]:
        assert STEPS in r and 'log_likelihood' not in r
        assert r[STEPS] == int(z['alb_MP_{}_steps'.format(r['method'])])
        assert hasattr(tree, r['character'])


# ---------------------------------------------------------------------------------------------------------------------
# 6. no likelihood buffers
def test_parsimony_only_context_holds_no_likelihood_buffers():
    """
    A tree-only context holds the tree's tables -- integers and one double per node, far less than one likelihood vector
    per node -- and pml_parsimony's scratch is at most 7 x n_cols N W 8 bytes (six arrays of sets and the int64 costs),
    released when the call returns: the context holds afterwards what it held before.
    """
    flat = FlatForest.balanced(18)   # 262 144 tips
    N, k, n_cols = flat.n_nodes, 20, 4
    given = random_given(flat, k, n_cols, seed=17)
    with hip.Engine.tree_only(flat) as eng:
        held0, free0 = eng.memory()
        sets, steps, hist = eng.parsimony(given, k, ALL_METHODS)
        held1, free1 = eng.memory()
    assert held1 == held0
    assert held0 < N * k * 8 * 2           # less than two columns of bottom-up vectors: there are none
    assert free0 - free1 <= 7 * n_cols * N * 8 + (64 << 20)   # (nothing of the scratch stays; the allocator may keep a little)
    assert hist.sum(axis=2).tolist() == [[N] * n_cols] * 3
    hs, hsteps, hhist = host_passes(flat, given[3], k)
    assert np.array_equal(masks_from_words(sets[:, 3], k), hs) and steps[:, 3].tolist() == hsteps.tolist()
