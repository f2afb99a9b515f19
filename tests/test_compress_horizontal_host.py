"""
CPU-only: the horizontal merging on the host (pastml_amd.visualisation.tree_compressor with device=False) and the Pajek writer
against what the reference's ``compress_tree(..., pajek_timing=HORIZONTAL)`` gave for the cases of
tests/golden/compress_horizontal.npz (make_golden_compress_horizontal.py, which asserts what each case is there for), line by
line; the switches of the second pass; the module's command line.  Integers and strings: every comparison is exact.
"""
import os

import numpy as np
import pytest

from conftest import REPO
from pastml_amd import pipeline
from pastml_amd.tree import FlatForest, StateSetColumn, read_tree
from pastml_amd.visualisation import tree_compressor as tc
from test_compress_host import CASES as VERTICAL_CASES, TABLE, TREE, load_case as load_vertical_case, pajek_text

GOLDEN = os.path.join(REPO, 'tests', 'golden', 'compress_horizontal.npz')
CASES = ['toy', 'widths', 'two_passes', 'decades', 'forest', 'albania']

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


def check_against_golden(merged, columns, expected, tmp_path):
    assert isinstance(merged, tc.HorizontalForest)
    vertices, arcs = tc.pajek_lines(merged, columns)
    assert vertices == [str(v) for v in expected['vertices']]
    assert arcs == [str(a) for a in expected['arcs']]
    assert np.array_equal(merged.width, expected['widths'])
    path = str(tmp_path / 'map.net')
    tc.save_to_pajek(merged, columns, path)
    with open(path) as f:
        assert f.read() == pajek_text(vertices, arcs)
    # the arrays agree with one another
    L = merged.n_vertices
    assert np.array_equal(np.diff(merged.member_offsets), merged.width) and merged.member_offsets[-1] == len(merged.members)
    assert np.array_equal(merged.members[merged.member_offsets[:-1]], merged.vertex)     # a vertex is its own first configuration
    assert (merged.parent < np.arange(L)).all() and (merged.width[merged.parent < 0] == 1).all()
    assert np.array_equal(np.add.reduceat(merged.compressed.n_tips_inside[merged.members], merged.member_offsets[:-1]),
                          merged.n_tips_total)
    assert np.array_equal(merged.second_pass, expected['passes'] == 2)


@pytest.mark.parametrize('case', CASES)
def test_host_path_reproduces_the_reference(case, tmp_path):
    flat, columns, column2states, expected = load_case(case)
    merged = tc.compress_forest(flat, columns, column2states, timing=tc.HORIZONTAL,
                                tip_size_threshold=int(expected['threshold']), device=False)
    check_against_golden(merged, columns, expected, tmp_path)


def test_goldens_hold_what_the_cases_are_for():
    g = golden()
    assert [str(a) for a in g['toy_arcs']][0] == '1 2 2' and sorted(g['toy_widths']) == [1, 1, 1, 1, 1, 1, 2]
    assert [str(v).split('"')[1] for v in g['widths_vertices']] == ['root', 'X', 'x1', 'Y', 'y1']
    assert g['widths_widths'].tolist() == [1, 2, 2, 1, 3]
    assert g['two_passes_passes'].tolist() == [2] and g['decades_passes'].tolist() == [2]
    assert [str(v).split('"')[1] for v in g['decades_vertices'][:4]] == ['root', 'n9', 'n10', 'n100']
    assert g['decades_widths'][:4].tolist() == [1, 1, 2, 1]
    assert g['forest_passes'].tolist() == [1, 2] and len(str(g['forest_newick']).split('\n')) == 2
    assert g['albania_widths'].max() > 1
    for case in CASES:   # the reference keys its cache by name: every node of every case has a name of its own
        flat = load_case(case)[0]
        names = [n.name for n in flat.nodes]
        assert all(names) and len(set(names)) == len(names)


def merged_of(case, **kwargs):
    flat, columns, column2states, expected = load_case(case)
    return tc.compress_forest(flat, columns, column2states, timing=tc.HORIZONTAL, device=False, **kwargs), expected


def test_member_order_of_the_toy():
    merged, _ = merged_of('toy')
    names = merged.compressed.name
    assert [list(names[merged.members[a:b]]) for a, b in zip(merged.member_offsets[:-1], merged.member_offsets[1:])] == \
        [['root'], ['p1', 'p2'], ['a1'], ['b1'], ['p3'], ['a3'], ['b3']]
    assert merged.merged_groups == [1, 0]


def test_decade_edges():
    """Leaf vertices of 9, 10, 99 and 100 tips: int(log10(.)) is 0, 1, 1, 2."""
    merged, _ = merged_of('decades')
    names = list(merged.compressed.name[merged.vertex])
    assert names[:4] == ['root', 'n9', 'n10', 'n100']
    assert merged.width[:4].tolist() == [1, 1, 2, 1] and merged.n_tips_total[:4].tolist() == [0, 9, 109, 100]
    assert merged.merged_groups == [0, 1]


def test_threshold_and_can_merge_diff_sizes_switch_the_second_pass():
    first_only, expected = merged_of('decades', can_merge_diff_sizes=False)
    assert first_only.merged_groups == [0, 0] and not first_only.second_pass.any()
    assert first_only.n_vertices == len(expected['vertices']) + 1          # n99 is still there
    # 24 leaf vertices after pass 1: a threshold of 24 is not exceeded, one of 23 is
    assert not merged_of('decades', tip_size_threshold=24)[0].second_pass.any()
    assert merged_of('decades', tip_size_threshold=23)[0].second_pass.all()
    # the small tree of the forest has 3 leaf vertices after pass 1 (a1, b1, a3)
    assert merged_of('forest', tip_size_threshold=2)[0].second_pass.tolist() == [True, True]
    assert merged_of('forest', tip_size_threshold=3)[0].second_pass.tolist() == [False, True]


def test_trim_is_refused_and_unknown_timings_are_errors():
    flat, columns, column2states, _ = load_case('toy')
    with pytest.raises(NotImplementedError, match='TRIM'):
        tc.compress_forest(flat, columns, column2states, timing=tc.TRIM, device=False)
    with pytest.raises(ValueError, match='timing'):
        tc.compress_forest(flat, columns, column2states, timing='SOMETIMES', device=False)


@pytest.mark.parametrize('case', VERTICAL_CASES)
def test_vertical_lines_are_unchanged(case):
    """compress_forest at VERTICAL is collapse_vertically, and its lines are those of compress_vertical.npz byte for byte."""
    flat, columns, column2states, expected = load_vertical_case(case)
    compressed = tc.compress_forest(flat, columns, column2states, device=False)
    assert isinstance(compressed, tc.CompressedForest)
    vertices, arcs = tc.pajek_lines(compressed, columns)
    assert pajek_text(vertices, arcs) == pajek_text([str(v) for v in expected['vertices']], [str(a) for a in expected['arcs']])


def test_pass_on_plain_arrays():
    """horizontal_pass_host on a hand-made vertex forest, dead vertices and vertices below a merged one included."""
    #        0
    #   1    2    3        1 and 2 are equal (children 4 ~ 5 under 1, 6 ~ 7 under 2), 3 is not live, 8 hangs under 3
    #  4 5  6 7   8
    parent = np.array([-1, 0, 0, 0, 1, 1, 2, 2, 3])
    live = np.array([1, 1, 1, 0, 1, 1, 1, 1, 0], dtype=bool)
    sets = np.ones((1, 9, 1), dtype=np.uint64)
    into, alive, width, groups = tc.horizontal_pass_host(parent, np.arange(9), np.zeros(9, int), np.ones(9, int), live, sets)
    assert into.tolist() == [0, 1, 1, 3, 4, 4, 6, 6, 8]
    assert alive.tolist() == [True, True, False, False, True, False, False, False, False]
    assert width.tolist() == [1, 2, 1, 1, 2, 1, 2, 1, 1] and groups == 3
    assert into.dtype == np.int32 and width.dtype == np.int32 and alive.dtype == bool
    # wide sets have no bound on the host: a difference in word 11 alone keeps 1 and 2 apart
    sets = np.ones((2, 9, 12), dtype=np.uint64)
    sets[1, 2, 11] = 3
    into, alive, width, groups = tc.horizontal_pass_host(parent, np.arange(9), np.zeros(9, int), np.ones(9, int), live, sets)
    assert into[2] == 2 and alive[[1, 2]].all() and groups == 2


def test_command_line_writes_the_map_of_a_run(tmp_path):
    """The pipeline's own output (COPY: no device) through the command line = compress_forest + save_to_pajek = the reference."""
    import pandas as pd
    from pastml_amd.acr import COPY
    from pastml_amd.annotation import preannotate_forest
    from pastml_amd.tree import read_forest
    work = str(tmp_path / 'work')
    pipeline.pastml_pipeline(TREE, data=TABLE, data_sep=',', columns=['Country'], prediction_method=COPY, work_dir=work)
    named_tree = os.path.join(work, pipeline.get_named_tree_file(TREE))
    table = os.path.join(work, pipeline.get_combined_ancestral_state_file())
    expected = load_case('albania')[3]
    for timing, lines in ((tc.HORIZONTAL, expected), (tc.VERTICAL, None)):
        out = str(tmp_path / (timing + '.net'))
        assert tc.main(['--tree', named_tree, '--states', table, '--pajek', out, '--pajek_timing', timing, '--host']) == 0
        roots = read_forest(named_tree)
        df = pd.read_csv(table, sep='\t', index_col=0, dtype=str, keep_default_na=False)
        preannotate_forest(roots, df=df)
        states = {'Country': np.array(sorted(set(df['Country']) - {''}))}
        direct = str(tmp_path / (timing + '.direct.net'))
        tc.save_to_pajek(tc.compress_forest(roots, ['Country'], states, timing=timing, device=False), ['Country'], direct)
        with open(out) as f, open(direct) as g:
            text = f.read()
            assert text == g.read()
        if lines is not None:
            assert text == pajek_text([str(v) for v in lines['vertices']], [str(a) for a in lines['arcs']])
    with pytest.raises(NotImplementedError, match='TRIM'):
        tc.main(['--tree', named_tree, '--states', table, '--pajek', str(tmp_path / 'trim.net'), '--pajek_timing', 'TRIM', '--host'])
