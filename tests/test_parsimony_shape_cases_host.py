"""
CPU tests of tests/parsimony_shape_cases.py, the inputs of tests/test_gpu_parsimony_shapes.py: the forests are what the fixture
(tests/golden/parsimony_shapes.npz, the reference's own results) was made on and need the counter widths the module states; the
host path of pastml_amd.parsimony reproduces the fixture exactly on every case -- unary nodes, lone tips and arities up to 256
included -- and the closed forms on the stars of 65534 and 65535 tips; the inputs do what they are for (a count of 2^P - 1, a tie
across the first and the last word, every W, a restricted unary node); and a restatement of the kernels' bit-sliced counters equals
the fixture with the right number of planes and differs from it with half of them or with a group OR that misses a word, so the
GPU file's assertions can fail.
"""
import numpy as np
import pytest

import parsimony_shape_cases as cases
from conftest import load_golden
from pastml_amd.batch import masks_from_words


@pytest.fixture(scope='module')
def golden():
    return load_golden('parsimony_shapes')


def _expected(z, name, k):
    return cases.fixture(z, name, k)


# ---------------------------------------------------------------------------------------------------------------------
# the forests and the fixture
def test_forests_are_those_of_the_fixture(golden):
    for name in cases.FIXTURE_FORESTS:
        assert np.array_equal(np.asarray(cases.forest(name).parent), golden[name + '_parent']), name
    for name, k in cases.FIXTURE_CASES:
        b, t = cases.build(name, k), cases.tag(name, k)
        assert b['cols'] == cases.columns_of(k) and golden[t + 'selected'].shape == b['given'].shape[:2] + (3, b['given'].shape[2])
        assert np.array_equal(golden[t + 'annotation'], b['given']), t
    stored = {key.rsplit('_', 1)[0] + '_' for key in golden.files if key.endswith('_annotation')}
    assert stored == {cases.tag(*c) for c in cases.FIXTURE_CASES}


def test_planes_of_every_forest():
    assert [cases.planes_for(a) for a in cases.ARITIES + cases.BIG_ARITIES] == [2, 4, 4, 8, 8, 16, 16, 16, 32]
    assert [cases.planes_for(a) for a in (0, 1, 2, 3, 14, 15, 254, 255, 65534, 65535, 1 << 30)] == [2, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    for name in cases.FORESTS:
        assert cases.planes_for(int(cases.forest(name).n_children.max())) == cases.PLANES[name], name
    assert [cases.PLANES[n] for n in cases.FORESTS[3:]] == [2, 4, 4, 8, 8, 16, 16, 16, 32]


@pytest.mark.parametrize('a', cases.ARITIES + cases.BIG_ARITIES)
def test_arity_forests_hold_what_they_name(a):
    flat = cases.forest('arity_{}'.format(a))
    nc, fc, roots = flat.n_children, flat.first_child, flat.roots
    assert nc.max() == a and nc[0] == a and flat.parent[0] < 0                      # a root star of a tips, the largest arity
    big = a in cases.BIG_ARITIES
    inner = [i for i in range(flat.n_nodes) if nc[i] == a and flat.parent[i] >= 0]
    assert len(inner) == (0 if big else 1)
    for i in inner:                                                                 # root -> [tip, inner node with a tips]
        p = flat.parent[i]
        assert flat.parent[p] < 0 and nc[p] == 2 and nc[fc[p]] == 0 and fc[p] + 1 == i
    for n in [0] + inner:
        assert np.all(nc[fc[n]:fc[n] + a] == 0)
    assert (nc[roots] == 0).sum() == 1                                              # a lone tip
    unary = np.flatnonzero(nc == 1)
    assert len(unary) == 2 and flat.parent[unary[0]] < 0 and flat.parent[unary[1]] == unary[0] and nc[fc[unary[1]]] == 0
    for s in (2, 3):
        if s <= a:
            assert any(nc[r] == s and np.all(nc[fc[r]:fc[r] + s] == 0) for r in roots)
    assert flat.n_nodes == (a + 12 if big else 2 * a + 15 - (4 if a < 3 else 0))
    assert flat.n_nodes < 1500 or (big and flat.n_nodes <= 65547)


def test_every_word_count_occurs():
    for name in ('shapes', 'grafted'):
        assert sorted({(k + 63) // 64 for k in cases.states_of(name)}) == list(range(1, 9))
    for name in cases.FORESTS:
        assert {(k + 63) // 64 for k in cases.states_of(name)} >= {1, 4, 8}          # WG = 1, 4 and 8; W = 4 has no dead lane ...
    assert 321 in cases.states_of('arity_255')                                      # ... W = 6 has two
    assert {k % 64 for k in cases.K_ALL} >= {0, 1}                                   # the last word full, and a single bit


# ---------------------------------------------------------------------------------------------------------------------
# the host path against the reference
@pytest.mark.parametrize('name,k', cases.FIXTURE_CASES, ids=cases.IDS)
def test_host_path_reproduces_the_fixture(golden, name, k):
    b = cases.build(name, k)
    sets, steps = _expected(golden, name, k)
    for c, col in enumerate(b['cols']):
        hs, hsteps = cases.host_passes(b['flat'], b['given'][c], k)
        assert np.array_equal(hs, masks_from_words(sets[:, c], k).astype(np.int8)), col
        assert hsteps.tolist() == steps[:, c].tolist(), col


def _is(words, states):
    want = np.zeros_like(words)
    cases._set_bits(want[None], 0, states)
    return np.array_equal(words, want)


@pytest.mark.parametrize('name', cases.BIG_FORESTS)
@pytest.mark.parametrize('k', cases.K_FEW)
def test_host_path_reproduces_the_closed_forms(name, k):
    b = cases.build(name, k)
    flat = b['flat']
    cases.assert_closed_forms(name, k, {col: cases.host_passes(flat, b['given'][col], k) for col in (0, 1, 2, 5)})


# ---------------------------------------------------------------------------------------------------------------------
# the inputs do what they are for
@pytest.mark.parametrize('name', cases.FORESTS)
def test_unanimous_column_counts_to_arity_plus_one(name):
    flat = cases.forest(name)
    a = int(flat.n_children.max())
    for k in cases.states_of(name) if name not in cases.BIG_FORESTS else cases.BIG_K_DEVICE:
        for n in cases.largest_nodes(flat):
            counts = cases.down_counts(flat, cases.build(name, k)['given'][0], k, n)
            assert counts[k - 1] == a + 1 and (k == 1 or counts[:k - 1].max() <= 1)
    assert a + 1 <= (1 << cases.PLANES[name]) - 1
    if a in (2, 14, 254, 65534):
        assert a + 1 == (1 << cases.PLANES[name]) - 1       # the counter is full: one more and it wraps to 0


# (every case that has column 2; the big forests at the state counts the device runs, by the host path)
TIE_CASES = [(n, k) for n, k in cases.CASES if k >= 2 and (n in cases.FIXTURE_FORESTS or k in cases.BIG_K_DEVICE)]


@pytest.mark.parametrize('name,k', TIE_CASES, ids=['{}-k{}'.format(*c) for c in TIE_CASES])
def test_tie_column_spans_the_first_and_the_last_word(golden, name, k):
    b = cases.build(name, k)
    flat, W = b['flat'], (k + 63) // 64
    if name in cases.FIXTURE_FORESTS:
        sets = _expected(golden, name, k)[0][:, 2]
    else:
        sets = cases.sets_as_words(cases.host_passes(flat, b['given'][2], k)[0], k)
    both = [int(r) for r in flat.roots if all(_is(sets[j, r], [0, k - 1]) for j in range(3))]
    assert both, 'no root with {s0, s1} under all three methods'
    if name.startswith('arity_'):
        assert 0 in both       # the root of the big star
    for r in both:
        assert sets[1, r, 0] & np.uint64(1) and sets[1, r, W - 1] >> np.uint64((k - 1) % 64) == 1


@pytest.mark.parametrize('name', cases.FORESTS)
def test_palette_column_restricts_a_unary_node_and_a_root(name):
    flat = cases.forest(name)
    nc = flat.n_children
    assert (nc == 1).any() and (nc[flat.roots] > 0).any()
    for k in cases.states_of(name):
        b = cases.build(name, k)
        given = b['given'][b['cols'].index(3)]
        u, r = b['restricted_unary'], b['restricted_root']
        assert nc[u] == 1 and given[u].any() and flat.parent[r] < 0 and nc[r] > 0 and given[r].any()
        pal = np.zeros((1, given.shape[1]), dtype=np.uint64)
        cases._set_bits(pal, 0, cases.palette(k))
        assert not (given & ~pal).any()
        sizes = masks_from_words(given, k).sum(axis=1)
        assert set(sizes[nc == 0].tolist()) <= {0, 1, min(3, len(cases.palette(k)))}
        assert set(sizes[nc > 0].tolist()) <= {0, min(2, len(cases.palette(k)))}


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: the kernels' counters restated
@pytest.mark.parametrize('name,k', cases.FIXTURE_CASES, ids=cases.IDS)
def test_restatement_equals_the_fixture_and_its_mutants_do_not(golden, name, k):
    b = cases.build(name, k)
    flat, W = b['flat'], (k + 63) // 64
    want_sets, want_steps = _expected(golden, name, k)
    sets, steps, down_max = cases.sliced_passes(flat, b['given'], k, cases.PLANES[name])
    assert np.array_equal(sets, want_sets) and np.array_equal(steps, want_steps)
    a = int(flat.n_children.max())
    assert np.all(down_max[0, cases.largest_nodes(flat)] == a + 1)

    def differing_columns(mutant):
        msets, msteps, _ = cases.mutant_passes(mutant, flat, b['given'], k)
        return [col for c, col in enumerate(b['cols'])
                if not (np.array_equal(msets[:, c], want_sets[:, c]) and np.array_equal(msteps[:, c], want_steps[:, c]))]
    if a >= 3:      # (two planes of a forest of at most two children: one plane still orders 0 < 1 and 2 < 3)
        assert 0 in differing_columns(cases.MUTANT_HALF_PLANES)
    if W > 1:
        assert differing_columns(cases.MUTANT_GROUP_OR)
    else:
        assert not differing_columns(cases.MUTANT_GROUP_OR)
