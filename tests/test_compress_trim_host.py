"""
CPU-only: the trimming on the host (pastml_amd.visualisation.tree_compressor with device=False) and the Pajek writer against
what the reference's ``compress_tree(..., pajek_timing=TRIM)`` gave for the cases of tests/golden/compress_trim.npz
(make_golden_compress_trim.py, which asserts what each case is there for): lines, thresholds, the numbers of vertices removed
and of mediators spliced out, the file; the module's command line; the refusals.  Every comparison is exact.
"""
import os

import numpy as np
import pytest

from conftest import REPO
from pastml_amd import pipeline
from pastml_amd.tree import FlatForest, StateSetColumn, read_tree
from pastml_amd.visualisation import tree_compressor as tc
from test_compress_host import CASES as VERTICAL_CASES, TABLE, TREE, load_case as load_vertical_case, pajek_text
from test_compress_horizontal_host import CASES as HORIZONTAL_CASES, load_case as load_horizontal_case

GOLDEN = os.path.join(REPO, 'tests', 'golden', 'compress_trim.npz')
CASES = ['under', 'no_small', 'plain', 'cascade', 'kept_internal', 'ties', 'mediator', 'chain3', 'order', 'barred', 'float_num',
         'final_merge', 'forest', 'ragged', 'albania']

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
    expected = {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(case + '_')}
    return flat, columns, column2states, expected


def trimmed_of(case, **kwargs):
    flat, columns, column2states, expected = load_case(case)
    kwargs.setdefault('device', False)
    result = tc.compress_tree(flat, columns, column2states, tip_size_threshold=int(expected['tip_size_threshold']),
                              can_merge_diff_sizes=bool(expected['can_merge']), **kwargs)
    return result, columns, expected


def check_against_golden(trimmed, columns, expected, tmp_path):
    assert isinstance(trimmed, tc.TrimmedForest) and isinstance(trimmed, tc.HorizontalForest)
    vertices, arcs = tc.pajek_lines(trimmed, columns)
    assert vertices == [str(v) for v in expected['vertices']]
    assert arcs == [str(a) for a in expected['arcs']]
    assert np.array_equal(trimmed.width, expected['widths'])
    assert np.array_equal(trimmed.threshold, expected['thresholds'], equal_nan=True) and trimmed.threshold.dtype == np.float64
    tree = trimmed.compressed.tree
    n_trees = len(expected['thresholds'])
    assert np.array_equal(np.bincount(tree[trimmed.removed], minlength=n_trees), expected['removed'])
    assert np.array_equal(np.bincount(tree[trimmed.mediators], minlength=n_trees), expected['mediators'])
    assert sorted(trimmed.compressed.name[trimmed.mediators]) == sorted(x for x in str(expected['mediator_names']).split(';') if x)
    assert len(trimmed.merged_groups) == 3 and trimmed.merged_groups[2] == int(expected['final_groups'].sum())
    path = str(tmp_path / 'map.net')
    tc.save_to_pajek(trimmed, columns, path)
    with open(path) as f:
        assert f.read() == pajek_text([str(v) for v in expected['vertices']], [str(a) for a in expected['arcs']])
    # the arrays agree with one another
    L = trimmed.n_vertices
    assert np.array_equal(np.diff(trimmed.member_offsets), trimmed.width) and trimmed.member_offsets[-1] == len(trimmed.members)
    assert np.array_equal(trimmed.members[trimmed.member_offsets[:-1]], trimmed.vertex)
    assert (trimmed.parent < np.arange(L)).all() and (trimmed.width[trimmed.parent < 0] == 1).all()
    assert np.array_equal(np.add.reduceat(trimmed.compressed.n_tips_inside[trimmed.members], trimmed.member_offsets[:-1]),
                          trimmed.n_tips_total)


@pytest.mark.parametrize('case', CASES)
def test_host_path_reproduces_the_reference(case, tmp_path):
    trimmed, columns, expected = trimmed_of(case)
    check_against_golden(trimmed, columns, expected, tmp_path)


def test_goldens_hold_what_the_cases_are_for():
    g = golden()
    names = lambda case: [str(v).split('"')[1] for v in g[case + '_vertices']]   # noqa: E731
    assert np.isnan(g['under_thresholds']).all() and np.isnan(g['no_small_thresholds']).all() and len(g['no_small_vertices']) == 5
    assert g['plain_removed'].tolist() == [2] and g['cascade_removed'].tolist() == [3] and names('cascade') == ['r', 'p', 'q', 's']
    assert names('kept_internal') == ['r', 'i', 'p', 'q'] and names('ties') == ['r', 'a', 'c', 'd', 'e']
    assert str(g['mediator_mediator_names']) == 'n' and names('mediator') == ['r', 'x', 'y', 'c']
    assert sorted(str(g['chain3_mediator_names']).split(';')) == ['n1', 'n3'] and names('chain3') == ['r', 'x', 'y', 'n2', 'c']
    assert names('order') == ['r', 'K', 'c1', 'c2'] and g['order_mediators'].tolist() == [2]
    assert g['barred_mediators'].tolist() == [0] and names('barred')[:5] == ['r', 'nT', 'cT', 'na', 'ca'] and g['barred_widths'][3] == 2
    assert not g['float_num_can_merge'] and g['float_num_final_groups'].tolist() == [1] and g['float_num_widths'][1] == 3
    assert g['final_merge_final_groups'].tolist() == [1] and g['final_merge_widths'][1] == 3
    assert np.isnan(g['forest_thresholds']).tolist() == [False, True]
    assert g['ragged_removed'][0] > 20 and g['albania_tip_size_threshold'] == 3 and not np.isnan(g['albania_thresholds'][0])
    for case in CASES:
        flat = load_case(case)[0]
        node_names = [n.name for n in flat.nodes]
        assert all(node_names) and len(set(node_names)) == len(node_names)


def test_trim_host_on_plain_arrays():
    """trim_host on a hand-made forest: dtypes, the tree that is not trimmed, the order of the outputs."""
    #  tree 0: 0 -> 1 (mediator {A,B}) -> 2 (B, 5 tips), 3 (small); 0 -> 4 (4 tips), 5 (3 tips)     tree 1: 6 -> 7
    parent = np.array([-1, 0, 1, 1, 0, 0, -1, 6])
    tree = np.array([0, 0, 0, 0, 0, 0, 1, 1])
    T = np.array([0, 0, 5, 1, 4, 3, 0, 1])
    w = np.ones(8, dtype=int)
    sets = np.array([[[1], [3], [2], [4], [8], [16], [1], [2]]], dtype=np.uint64)
    tsize, keep, spliced, new_parent, moved, threshold = tc.trim_host(parent, tree, T, w, sets, 3, [True, False])
    assert tsize.tolist() == [0, 0, 5, 1, 4, 3, 0, 0] and threshold[0] == 3 and np.isnan(threshold[1])
    assert keep.tolist() == [True, True, True, False, True, True, True, True]
    assert spliced.tolist() == [False, True] + [False] * 6
    assert new_parent.tolist() == [-1, -1, 0, -1, 0, 0, -1, 6] and moved.tolist() == [False, False, True] + [False] * 5
    assert (tsize.dtype, keep.dtype, spliced.dtype, new_parent.dtype, moved.dtype, threshold.dtype) == \
        (np.float64, bool, bool, np.int32, bool, np.float64)
    # k = 0 selects the minimum: nothing is trimmed
    assert np.isnan(tc.trim_host(parent, tree, T, w, sets, 0, [True, True])[5]).all()
    # no bound on W on the host: the mediator fails on word 11 alone
    wide = np.zeros((1, 8, 12), dtype=np.uint64)
    wide[:, :, :1] = sets
    wide[0, 1, 11] = 1
    assert not tc.trim_host(parent, tree, T, w, wide, 3, [True, False])[2].any()
    for bad in (dict(parent=[-1, 0, 1, 1, 0, 0, -1, 7]), dict(w=[1, 1, 0, 1, 1, 1, 1, 1]), dict(T=[0, 0, 5, -1, 4, 3, 0, 1]),
                dict(parent=[-1, 0, 1, 0, 1, 0, -1, 6])):
        args = dict(parent=parent, tree=tree, T=T, w=w)
        args.update(bad)
        with pytest.raises(ValueError):
            tc.trim_host(args['parent'], args['tree'], args['T'], args['w'], sets, 3, [True, False])


@pytest.mark.parametrize('case', HORIZONTAL_CASES)
def test_horizontal_through_compress_tree_is_compress_forest(case):
    flat, columns, column2states, expected = load_horizontal_case(case)
    k = int(expected['threshold'])
    one = tc.compress_tree(flat, columns, column2states, tip_size_threshold=k, pajek_timing=tc.HORIZONTAL, device=False)
    other = tc.compress_forest(flat, columns, column2states, timing=tc.HORIZONTAL, tip_size_threshold=k, device=False)
    assert type(one) is tc.HorizontalForest and tc.pajek_lines(one, columns) == tc.pajek_lines(other, columns)
    assert tc.pajek_lines(one, columns)[0] == [str(v) for v in expected['vertices']]


@pytest.mark.parametrize('case', VERTICAL_CASES)
def test_vertical_through_compress_tree_is_compress_forest(case):
    flat, columns, column2states, expected = load_vertical_case(case)
    one = tc.compress_tree(flat, columns, column2states, pajek_timing=tc.VERTICAL, device=False)
    assert type(one) is tc.CompressedForest
    assert tc.pajek_lines(one, columns) == tc.pajek_lines(tc.compress_forest(flat, columns, column2states, device=False), columns)
    assert tc.pajek_lines(one, columns)[0] == [str(v) for v in expected['vertices']]


def test_bad_arguments():
    flat, columns, column2states, _ = load_case('plain')
    with pytest.raises(ValueError, match='negative'):
        tc.compress_tree(flat, columns, column2states, tip_size_threshold=-1, device=False)
    merged = tc.compress_forest(flat, columns, column2states, timing=tc.HORIZONTAL, device=False)
    with pytest.raises(ValueError, match='negative'):
        tc.trim(merged, tip_size_threshold=-1, device=False)
    with pytest.raises(ValueError, match='pajek_timing'):
        tc.compress_tree(flat, columns, column2states, pajek_timing='SOMETIMES', device=False)
    # the pinned refusal stays, and says where the trimmed forest is
    with pytest.raises(NotImplementedError, match='TRIM.*compress_tree'):
        tc.compress_forest(flat, columns, column2states, timing=tc.TRIM, device=False)


def test_multiplier_overflow_raises():
    """Widths of 2^20 down a path of three: 2^60.  Python's unbounded integers are not reproduced."""
    parent = np.array([-1, 0, 1, 2, 0, 0])
    w = np.array([1, 2 ** 20, 2 ** 20, 2 ** 20, 1, 1])
    T = np.array([0, 0, 0, 1, 2, 3])
    sets = np.arange(1, 7, dtype=np.uint64).reshape(1, 6, 1)
    with pytest.raises(ValueError, match='2\\^53'):
        tc.trim_host(parent, np.zeros(6, int), T, w, sets, 2, [True])
    assert np.isnan(tc.trim_host(parent, np.zeros(6, int), T, w, sets, 2, [False])[5]).all()    # (not asked to trim: no sizes)
    w[1] = 2 ** 12                                                        # a multiplier of 2^52 is fine: (1 / 2^20) * 2^52
    assert tc.trim_host(parent, np.zeros(6, int), T, w, sets, 2, [True])[0][3] == 2.0 ** 32


def test_command_line_writes_the_trimmed_map_of_a_run(tmp_path):
    """The pipeline's own output (COPY: no device) through ``--trim --host`` = compress_tree + save_to_pajek = the reference."""
    from pastml_amd.acr import COPY
    work = str(tmp_path / 'work')
    pipeline.pastml_pipeline(TREE, data=TABLE, data_sep=',', columns=['Country'], prediction_method=COPY, work_dir=work)
    named_tree = os.path.join(work, pipeline.get_named_tree_file(TREE))
    table = os.path.join(work, pipeline.get_combined_ancestral_state_file())
    expected = load_case('albania')[3]
    out = str(tmp_path / 'trim.net')
    assert tc.main(['--tree', named_tree, '--states', table, '--pajek', out, '--trim', '--tip_size_threshold', '3', '--host']) == 0
    with open(out) as f:
        assert f.read() == pajek_text([str(v) for v in expected['vertices']], [str(a) for a in expected['arcs']])
    with pytest.raises(SystemExit):
        tc.main(['--tree', named_tree, '--states', table, '--pajek', out, '--trim', '--pajek_timing', 'HORIZONTAL', '--host'])
