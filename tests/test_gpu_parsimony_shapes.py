"""
The parsimony passes on the device (pml_parsimony) at every counter width, on every lane group and on degenerate forests: the cases of
tests/parsimony_shape_cases.py against the reference's pastml/parsimony.py (tests/golden/parsimony_shapes.npz) -- forests whose
largest arity sits on either side of 14 / 15 and 254 / 255, inputs whose winning count fills the counter (2^P - 1), ties and winners
across the first and the last word of a set, W = 1 .. 8 words with dead lanes at 3, 5, 6 and 7, unary nodes, lone tips, roots over one
tip and stars -- and, for the stars of 65534 and 65535 tips, against closed forms and the host path, which
tests/test_parsimony_shape_cases_host.py pins to the same fixture.  That file also shows that these comparisons fail for counters of
half the planes and for a group OR that misses a word.  Integer work: every comparison is exact; no case is filtered.
"""
import numpy as np
import pytest

import parsimony_shape_cases as cases
from conftest import load_golden
from pastml_amd import hip
from pastml_amd import parsimony as P
from pastml_amd.batch import masks_from_words
from pastml_amd.parsimony import STEPS
from pastml_amd.tree import FlatForest, get_flat_forest

pytestmark = pytest.mark.gpu
ALL_METHODS = hip.PARS_ACCTRAN | hip.PARS_DOWNPASS | hip.PARS_DELTRAN


@pytest.fixture(scope='module')
def golden():
    return load_golden('parsimony_shapes')


def device(name, k, tune=None, methods=ALL_METHODS):
    b = cases.build(name, k)
    with hip.Engine.tree_only(b['flat'], tune=tune) as eng:
        return eng.parsimony(b['given'], k, methods)


def size_histogram(sets, k):
    """[..., k + 1]: nodes by the number of states of their set; sets uint64 [..., N, W]."""
    sizes = masks_from_words(sets, k).sum(axis=-1)
    flat_sizes = sizes.reshape(-1, sizes.shape[-1])
    return np.stack([np.bincount(row, minlength=k + 1) for row in flat_sizes]).reshape(sizes.shape[:-1] + (k + 1,))


def assert_equals_fixture(out, golden, name, k):
    want_sets, want_steps = cases.fixture(golden, name, k)
    sets, steps, hist = out
    for j, method in enumerate(cases.METHODS):
        for c, col in enumerate(cases.columns_of(k)):
            assert np.array_equal(sets[j, c], want_sets[j, c]), (method, col)
    assert np.array_equal(steps, want_steps)
    assert np.array_equal(hist, size_histogram(want_sets, k))


def assert_same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every case against the reference
@pytest.mark.parametrize('name,k', cases.FIXTURE_CASES, ids=cases.IDS)
def test_device_matches_reference(golden, name, k):
    assert np.array_equal(np.asarray(cases.forest(name).parent), golden[name + '_parent'])
    assert np.array_equal(cases.build(name, k)['given'], golden[cases.tag(name, k) + 'annotation'])
    assert_equals_fixture(device(name, k), golden, name, k)


# ---------------------------------------------------------------------------------------------------------------------
# 2. 16 planes filled to 2^16 - 1, and 32 planes: beyond the reference's reach
@pytest.mark.parametrize('name', cases.BIG_FORESTS)
@pytest.mark.parametrize('k', cases.BIG_K_DEVICE)
def test_big_stars_match_closed_forms_and_host_path(name, k):
    b = cases.build(name, k)
    flat = b['flat']
    sets, steps, hist = device(name, k)
    as_masks = masks_from_words(sets, k).astype(np.int8)
    cases.assert_closed_forms(name, k, {col: (as_masks[:, col], steps[:, col]) for col in (0, 1, 2, 5)})
    for c in b['cols']:
        hs, hsteps = cases.host_passes(flat, b['given'][c], k)
        assert np.array_equal(as_masks[:, c], hs), c
        assert steps[:, c].tolist() == hsteps.tolist(), c
    assert np.array_equal(hist, size_histogram(sets, k)) and np.all(hist.sum(axis=2) == flat.n_nodes)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the level schedule: every level its own launch, the default, the whole pass in one workgroup per column
@pytest.mark.parametrize('name', ['crowd', 'grafted', 'arity_255'])
def test_launch_schedule_is_invisible(golden, name):
    k = 193
    launches = []
    for tune in (dict(PARS_THIN=1), None, dict(PARS_THIN=1 << 30)):
        b = cases.build(name, k)
        with hip.Engine.tree_only(b['flat'], tune=tune) as eng:
            out = eng.parsimony(b['given'], k, ALL_METHODS)
            launches.append(eng.parsimony_info()[0])
        assert_equals_fixture(out, golden, name, k)
    # (a level of one unit still shares a launch at PARS_THIN = 1: no more launches with larger limits, fewer on a forest with
    # levels of several units)
    assert launches[0] >= launches[1] >= launches[2] and launches[0] > launches[2]


# ---------------------------------------------------------------------------------------------------------------------
# 4. column chunks, numbering, method subsets
def test_column_chunks_of_one(golden):
    name, k = 'grafted', 321
    whole = device(name, k)
    assert_equals_fixture(whole, golden, name, k)
    assert_same(device(name, k, tune=dict(PARS_MAX_COLS=1)), whole)


@pytest.mark.parametrize('name', ['shapes', 'grafted'])
def test_numbering_is_invisible(golden, name):
    k = 321
    for tune in (None, dict(NO_HEIGHT_ORDER=1), dict(SHAPE_ORDER=1)):
        assert_equals_fixture(device(name, k, tune=tune), golden, name, k)


@pytest.mark.parametrize('methods', [1, 2, 3, 4, 5, 6])
def test_method_subsets_fill_their_slots(golden, methods):
    name, k = 'shapes', 129
    want_sets, want_steps = cases.fixture(golden, name, k)
    slots = [j for j in range(3) if methods >> j & 1]
    sets, steps, hist = device(name, k, methods=methods)   # (DELTRAN alone still runs DOWN)
    assert sets.shape[0] == len(slots)
    assert np.array_equal(sets, want_sets[slots]) and np.array_equal(steps, want_steps[slots])
    assert np.array_equal(hist, size_histogram(want_sets[slots], k))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the acr-level path: result dictionaries and node features
@pytest.mark.parametrize('k', cases.states_of('shapes'))
def test_acr_batch_matches_reference_results(golden, k):
    z = golden
    b = cases.build('shapes', k)
    shared = b['flat']
    flat = FlatForest(shared.parent, shared.n_children, shared.first_child, shared.dist, shared.roots)   # (features stay off the shared forest)
    roots = flat.to_tree_nodes()
    row = z['shapes_c3_k'].tolist().index(k)
    c = b['cols'].index(3)
    states = np.array(['s{:03d}'.format(i) for i in range(k)])
    ann = masks_from_words(b['given'][c], k).astype(bool)
    want_sets, _ = cases.fixture(z, 'shapes', k)
    order = list(zip(z['shapes_c3_prediction_method'], z['shapes_c3_method'], z['shapes_c3_character']))
    seen = 0
    for method in (P.MP, P.DOWNPASS, P.ACCTRAN, P.DELTRAN):
        for i, n in enumerate(flat.nodes):
            if ann[i].any():
                n.add_feature('ch', set(states[ann[i]]))
            else:
                n.del_feature('ch')
        results, = P.parsimonious_acr_batch(roots, ['ch'], [method], [states], flat.n_nodes, flat.n_tips)
        columns = get_flat_forest(roots).columns
        for r in results:
            assert (method, r['method'], r['character']) == tuple(str(v) for v in order[seen])
            assert r[STEPS] == int(z['shapes_c3_steps'][row, seen])
            assert str(r['num_scenarios']) == str(z['shapes_c3_num_scenarios'][row, seen])
            assert r['num_unresolved_nodes'] == int(z['shapes_c3_num_unresolved_nodes'][row, seen])
            assert r['num_states_per_node_avg'] == float(z['shapes_c3_num_states_per_node_avg'][row, seen])
            assert r['num_nodes'] == flat.n_nodes and r['num_tips'] == flat.n_tips
            assert np.array_equal(columns[r['character']].words, want_sets[cases.METHODS.index(r['method']), c]), (method, r['method'])
            seen += 1
    assert seen == len(order) == 6
