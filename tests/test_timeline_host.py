"""
CPU-only: the dates (pastml_amd.tree.annotate_dates) and the timeline on the host (pastml_amd.visualisation.timeline with
device=False) against what the reference's ``annotate_dates``, ``visualize``, ``update_milestones`` and
``_forest2json_compressed`` gave for the cases of tests/golden/timeline.npz (make_golden_timeline.py, which asserts what each
case is there for): every node's date bit for bit, the milestones, the labels, MILESTONE and the texts of every vertex and
milestone string for string; the table writer; the refusals.  Every comparison is exact.

Labels: where the dates are no calendar dates the reference keeps the labels of the milestones it chose BEFORE
``update_milestones`` changed them (``update_milestones`` re-labels calendar dates only), so a trimmed case may carry more labels
than milestones.  Here the labels are always those of the milestones; such a case is compared with ``'{:g}'`` of the golden
milestones, every other one with the golden labels.
"""
import os

import numpy as np
import pytest

from conftest import REPO
from pastml_amd.tree import ArrayColumn, FlatForest, IS_POLYTOMY, StateSetColumn, annotate_dates, read_tree
from pastml_amd import tree as our_tree
from pastml_amd.visualisation import timeline as tl
from pastml_amd.visualisation import tree_compressor as tc

GOLDEN = os.path.join(REPO, 'tests', 'golden', 'timeline.npz')
CASES = ['forest_dates', 'shared_SAMPLED', 'shared_NODES', 'shared_LTT', 'polytomy', 'min_max', 'internal_as_tip', 'trimmed',
         'trimmed_NODES', 'trimmed_LTT', 'milestones', 'one_milestone', 'ragged_SAMPLED', 'ragged_NODES', 'ragged_LTT']
ABSENT = '<absent>'
TEXTS = (('tips_inside', 'node_' + tl.TIPS_INSIDE), ('internal_inside', 'node_' + tl.INTERNAL_NODES_INSIDE),
         ('tips_below', 'node_' + tl.TIPS_BELOW), ('edge_name', tl.EDGE_NAME))

_golden = []


def golden():
    if not _golden:
        _golden.append(dict(np.load(GOLDEN)))
    return _golden[0]


def load_case(case):
    """(flat forest with the case's columns set, columns, column -> states, golden arrays of the case)."""
    g = golden()
    roots = [read_tree(nwk) for nwk in str(g[case + '_newick']).split('\n')]
    flat = FlatForest.from_trees(roots)
    columns = [str(c) for c in g[case + '_columns']]
    column2states = {}
    for i, c in enumerate(columns):
        column2states[c] = g['{}_states_{}'.format(case, i)]
        flat.set_column(c, StateSetColumn(g['{}_words_{}'.format(case, i)], column2states[c]))
    flags = g[case + '_polytomy']
    if flags.any():
        col = ArrayColumn(np.ones(flat.n_nodes, dtype=np.int8), convert=int)
        col.absent = ~flags
        flat.set_column(IS_POLYTOMY, col)
    expected = {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(case + '_')}
    return flat, columns, column2states, expected


def dates_of(expected):
    """(root_dates or None, given or None) as the case was run."""
    roots = expected['root_dates']
    given = expected['given']
    return (None if np.isnan(roots).all() else roots.tolist()), (None if np.isnan(given).all() else given)


def timeline_of(case, device=False, **kwargs):
    flat, columns, column2states, expected = load_case(case)
    compressed = tc.compress_tree(flat, columns, column2states, tip_size_threshold=int(expected['tip_size_threshold']), device=device)
    root_dates, given = dates_of(expected)
    result = tl.timeline(compressed, root_dates=root_dates, given_dates=given, timeline_type=str(expected['timeline_type']),
                         dates_are_dates=bool(expected['dates_are_dates']), device=device, **kwargs)
    return result, compressed, expected


def check_against_golden(result, compressed, expected):
    assert result.date.dtype == np.float64 and np.array_equal(result.date.view(np.int64), expected['date'].view(np.int64))
    assert np.array_equal(result.milestones.view(np.int64), expected['milestones'].view(np.int64))
    M, L = len(expected['milestones']), len(expected['vertex_names'])
    labels = [str(x) for x in expected['labels']]
    if not bool(expected['dates_are_dates']):
        labels = ['{:g}'.format(m) for m in expected['milestones']]   # (stale in the reference: see the module docstring)
    assert result.labels == labels
    assert [str(x) for x in compressed.compressed.name[compressed.vertex]] == [str(x) for x in expected['vertex_names']]
    assert result.n_vertices == L and result.n_roots.shape == (L, M)
    features = result.features()
    for v in range(L):
        want = {}
        if expected['mile'][v] >= 0:
            want[tl.MILESTONE] = int(expected['mile'][v])
        for key, feature in TEXTS:
            for i in range(M):
                if str(expected[key][v, i]) != ABSENT:
                    want['{}_{}'.format(feature, i)] = str(expected[key][v, i])
        assert features[v] == want, (v, expected['vertex_names'][v])
        assert result.features(v) == want
    assert np.array_equal(result.first_milestone, expected['mile'] if M > 1 else np.zeros(L))
    for name in tl.COUNTS:
        assert getattr(result, name).dtype == np.int32


@pytest.mark.parametrize('case', CASES)
def test_host_path_reproduces_the_reference(case):
    result, compressed, expected = timeline_of(case)
    check_against_golden(result, compressed, expected)


@pytest.mark.parametrize('case', CASES)
def test_annotate_dates_carries_the_bits_of_the_reference(case):
    flat, _, _, expected = load_case(case)
    root_dates, given = dates_of(expected)
    date = annotate_dates(flat, root_dates, given)
    assert np.array_equal(date.view(np.int64), expected['date'].view(np.int64))


def test_goldens_hold_what_the_cases_are_for():
    g = golden()
    assert len(g['forest_dates_root_dates']) == 2 and not np.isnan(g['forest_dates_given']).all() and g['forest_dates_dates_are_dates']
    assert len(g['one_milestone_milestones']) == 1 and (g['one_milestone_mile'] == -1).all()
    assert g['polytomy_polytomy'].sum() == 1
    assert any('-' in str(x) for x in g['min_max_tips_inside'].ravel())
    assert len(g['trimmed_labels']) != len(g['trimmed_milestones'])   # (the stale labels of the reference)
    assert str(g['trimmed_tips_below'][0, -1]) == ' 14' and sum(int(x) for x in g['trimmed_tips_inside'][:, -1]) == 12
    assert (g['shared_NODES_tips_inside'] != g['shared_LTT_tips_inside']).any()
    assert set(g['shared_NODES_date'].tolist()) & set(g['shared_NODES_milestones'].tolist())


def test_a_single_milestone_gives_arrays_and_no_features():
    result, compressed, expected = timeline_of('one_milestone')
    assert result.features() == [{}] * result.n_vertices
    assert (result.first_milestone == 0).all() and (result.n_roots == 1).all()
    assert result.tips_max.sum() == 4 and result.below_max[0, 0] == 4


def test_given_milestones_and_the_table(tmp_path):
    result, compressed, expected = timeline_of('trimmed', milestones=[1., 3., 100.])
    assert result.labels == ['1', '3', '100'] and result.n_roots.shape == (4, 3)
    # at the end everything is shown: 12 tips are left inside, all 15 are below the root
    assert result.tips_max[:, 2].sum() == 12 and result.below_max[0, 2] == 15
    # nothing is sampled before 1.4: no vertex exists at the first milestone, and no row is written for it
    assert (result.n_roots[:, 0] == 0).all() and (result.below_max[:, 0] == 0).all() and (result.first_milestone == 1).all()
    path = str(tmp_path / 'timeline.tab')
    tl.write_timeline(result, compressed, path)
    with open(path) as f:
        lines = f.read().split('\n')
    assert lines[0] == 'milestone\tid\tvertex\troots\ttips_inside\tinternal_nodes_inside\ttips_below' and lines[-1] == ''
    rows = [line.split('\t') for line in lines[1:-1]]
    assert len(rows) == int((result.n_roots > 0).sum())
    assert rows[-1] == ['100', '4', 'c', '1', '5', '1', '5'] and rows[0] == ['3', '1', 'r', '1', '0', '1', '7']


def test_vertical_and_horizontal_forests_are_taken():
    flat, columns, column2states, expected = load_case('min_max')
    for timing in (tc.VERTICAL, tc.HORIZONTAL):
        compressed = tc.compress_tree(flat, columns, column2states, tip_size_threshold=2, pajek_timing=timing, device=False)
        result = tl.timeline(compressed, device=False)
        assert result.alive.all() and result.tips_max[:, -1].sum() >= 7
        assert result.n_vertices == (compressed.n_vertices if timing == tc.VERTICAL else len(compressed.vertex))
    # one configuration per vertex: minimum and maximum agree everywhere
    vertical = tl.timeline(tc.compress_tree(flat, columns, column2states, pajek_timing=tc.VERTICAL, device=False), device=False)
    assert np.array_equal(vertical.tips_min, vertical.tips_max) and vertical.n_roots.max() == 1
    assert vertical.tips_max[:, -1].sum() == 21


def test_refusals():
    flat, columns, column2states, expected = load_case('shared_NODES')
    compressed = tc.compress_tree(flat, columns, column2states, device=False)
    with pytest.raises(ValueError, match='at most 64'):
        tl.timeline(compressed, milestones=np.arange(65.), device=False)
    assert len(tl.timeline_host(tl.timeline_arrays(compressed), milestones=np.arange(65.))['milestones']) == 65   # (no bound there)
    with pytest.raises(ValueError, match='ascending'):
        tl.timeline(compressed, milestones=[2., 1.], device=False)
    with pytest.raises(ValueError, match='ascending'):
        tl.timeline(compressed, milestones=[1., 1.], device=False)
    with pytest.raises(ValueError, match='Unknown timeline type'):
        tl.timeline(compressed, timeline_type='TIPS', device=False)
    # a given date before the parent's: get_date decreases, and the node is named
    given = np.full(flat.n_nodes, np.nan)
    given[[n.name for n in flat.nodes].index('f')] = 0.5
    with pytest.raises(ValueError, match="decreases from node 'l'.*to its child 'f'"):
        tl.timeline(compressed, given_dates=given, timeline_type='NODES', device=False)
    given = np.full(flat.n_nodes, np.nan)
    given[[n.name for n in flat.nodes].index('k')] = -1.
    with pytest.raises(ValueError, match="decreases from node 'l'.*to its child 'k'"):
        tl.timeline(compressed, given_dates=given, timeline_type='LTT', device=False)
    with pytest.raises(ValueError, match='root dates'):
        annotate_dates(flat, root_dates=[1., 2.])


def test_dates_parse_and_convert():
    assert our_tree.parse_date('2016.5') == 2016.5 and our_tree.parse_date(3) == 3.
    assert our_tree.datetime2numeric(our_tree.numeric2datetime(2016.9972677595629)) == 2016.9972677595629
    assert our_tree.numeric2datetime(2016.0).strftime('%d %b %Y') == '01 Jan 2016'
    assert our_tree.parse_date('2016-12-31') == 2016.9972677595629
    with pytest.raises(ValueError, match='Could not infer'):
        our_tree.parse_date('no date')
    assert tl.milestone_labels([2016.0, 1e9], True) == ['2016', '1e+09']   # (a year no datetime holds: the numbers are shown)
