"""
CPU-only: the vertical collapse on the host (pastml_amd.visualisation.tree_compressor with device=False) and the Pajek
writer against what the reference's tree compressor gave for the cases of tests/golden/compress_vertical.npz
(make_golden_compress.py), byte for byte; the argument handling of the pipeline.
"""
import os

import numpy as np
import pytest

from conftest import REPO
from pastml_amd import pipeline
from pastml_amd.tree import ArrayColumn, FlatForest, IS_POLYTOMY, StateSetColumn, read_tree
from pastml_amd.visualisation import tree_compressor as tc

GOLDEN = os.path.join(REPO, 'tests', 'golden', 'compress_vertical.npz')
CASES = ['toy', 'ragged', 'forest', 'last_word', 'resolved']
TREE = os.path.join(REPO, 'tests', 'golden', 'data', 'Albanian.tree.152tax.tre')
TABLE = os.path.join(REPO, 'tests', 'golden', 'data', 'data.txt')

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


def pajek_text(vertices, arcs):
    return '*vertices {}\n{}\n*arcs\n{}'.format(len(vertices), '\n'.join(vertices), '\n'.join(arcs))


def check_against_golden(compressed, columns, expected, tmp_path):
    by_rank = np.argsort(compressed.order)
    assert np.array_equal(np.sort(compressed.order), np.arange(compressed.n_vertices))
    assert np.array_equal(compressed.n_tips_inside[by_rank], expected['tips_inside'])
    assert np.array_equal(compressed.n_internal_inside[by_rank], expected['internal_inside'])
    path = str(tmp_path / 'map.net')
    tc.save_to_pajek(compressed, columns, path)
    with open(path) as f:
        text = f.read()
    assert text == pajek_text([str(v) for v in expected['vertices']], [str(a) for a in expected['arcs']])
    # the arrays agree with one another
    assert np.array_equal(compressed.top[compressed.vertex_of_node[compressed.top]], compressed.top)
    assert (compressed.parent[compressed.parent < 0] == -1).all()
    assert np.array_equal(np.bincount(compressed.vertex_of_node[compressed.flat.tips], minlength=compressed.n_vertices),
                          compressed.n_tips_inside)


@pytest.mark.parametrize('case', CASES)
def test_host_path_reproduces_the_reference(case, tmp_path):
    flat, columns, column2states, expected = load_case(case)
    compressed = tc.collapse_vertically(flat, columns, column2states, device=False)
    check_against_golden(compressed, columns, expected, tmp_path)


def test_goldens_hold_what_the_cases_are_for():
    g = golden()
    assert g['ragged_words_2'].shape[1] == 2 and g['ragged_words_0'].shape[1] == 1       # W = 2 with padding
    assert len(g['ragged_states_0']) == 4 and len(g['ragged_states_1']) == 20 and len(g['ragged_states_2']) == 70
    assert len(str(g['forest_newick']).split('\n')) == 2
    assert g['last_word_words_1'].shape[1] == 3 and len(g['last_word_states_1']) == 130
    assert g['resolved_polytomy'].sum() > 0
    # polytomy nodes are left out of the internal nodes inside: every other node is a tip or an internal node of some vertex.
    # (The reference copies onto its compressed tree only the features its ROOT carries, so on what resolve_trees leaves it
    # would count them; make_golden_compress.py gives the root of this case polytomy = 0 so that the flags are seen and
    # tree_compressor.py:94 does what it is written for.  The golden count is the reference's on that adjusted input.)
    n = len(g['resolved_polytomy'])
    assert g['resolved_tips_inside'].sum() + g['resolved_internal_inside'].sum() == n - g['resolved_polytomy'].sum()
    # last_word: two nodes differ from their parents in nothing but the last word of the last column
    flat, columns, _, _ = load_case('last_word')
    w0, w1 = g['last_word_words_0'], g['last_word_words_1']
    has_parent = flat.parent >= 0
    up = np.maximum(flat.parent, 0)
    only_last = has_parent & (w0 == w0[up]).all(axis=1) & (w1[:, :2] == w1[up][:, :2]).all(axis=1) & (w1[:, 2] != w1[up][:, 2])
    assert only_last.sum() >= 2


def test_toy_example_written_out(tmp_path):
    """The example of the reference run: it pins the order of a vertex's children (n2 before x) and the ';' between tips."""
    root = read_tree('((a:1,b:1,(c:1,d:0)x:1)n1:1,(e:1,(f:1,g:1)n3:0.5)n2:1,h:2)root;')
    for node in root.traverse():
        node.add_feature('c2', {'X'})
        node.add_feature('col', {'B'} if node.name in ('c', 'e', 'f', 'n3', 'n2') else {'A'})
        if node.name == 'x':
            node.add_feature('col', {'A', 'B'})
    compressed = tc.collapse_vertically(root, ['col', 'c2'], device=False)
    path = str(tmp_path / 'toy.net')
    tc.save_to_pajek(compressed, ['col', 'c2'], path)
    with open(path) as f:
        text = f.read()
    assert text == ('*vertices 6\n'
                    '1 "root" "a;b;h" "c2:X" "col:A"\n'
                    '2 "n2" "e;f" "c2:X" "col:B"\n'
                    '3 "g" "g" "c2:X" "col:A"\n'
                    '4 "x" "" "c2:X" "col:A or B"\n'
                    '5 "c" "c" "c2:X" "col:B"\n'
                    '6 "d" "d" "c2:X" "col:A"\n'
                    '*arcs\n'
                    '1 2 1\n2 3 1\n1 4 1\n4 5 1\n4 6 1')
    by_rank = np.argsort(compressed.order)
    assert list(compressed.name[by_rank]) == ['root', 'n2', 'g', 'x', 'c', 'd']
    assert list(compressed.n_tips_inside[by_rank]) == [3, 2, 1, 0, 1, 1]
    assert list(compressed.n_internal_inside[by_rank]) == [2, 2, 0, 1, 0, 0]
    assert list(compressed.order[compressed.parent[by_rank]][1:]) == [0, 1, 0, 3, 3]
    names = np.array([n.name for n in compressed.flat.nodes])
    assert sorted(names[compressed.vertex_of_node == compressed.vertex_of_node[0]]) == ['a', 'b', 'h', 'n1', 'root']


def test_missing_feature_is_the_empty_set():
    """A node without the feature merges into a parent without it, and not into one that has a state."""
    root = read_tree('((a:1,b:1)n1:1,c:1)root;')
    for node in root.traverse():
        if node.name in ('root', 'c'):
            node.add_feature('col', {'A'})
    compressed = tc.collapse_vertically(root, ['col'], device=False)
    by_rank = np.argsort(compressed.order)
    assert list(compressed.name[by_rank]) == ['root', 'n1']
    assert list(compressed.n_tips_inside[by_rank]) == [1, 2]
    vertices, arcs = tc.pajek_lines(compressed)
    assert vertices == ['1 "root" "c" "col:A"', '2 "n1" "a;b" "col:"'] and arcs == ['1 2 1']


def test_jump_rounds_cover_the_depth():
    assert [tc.jump_rounds(d) for d in (0, 1, 2, 3, 4, 5, 1024, 1025)] == [0, 0, 1, 2, 2, 3, 10, 11]
    # a caterpillar: as many levels as tips, one vertex
    n = 300
    newick = 't0:1'
    for i in range(1, n):
        newick = '({},t{}:1)n{}:1'.format(newick, i, i)
    root = read_tree(newick + ';')
    flat = FlatForest.from_trees([root])
    assert flat.n_td_levels == n and flat.n_nodes == 2 * n - 1
    sets = np.ones((1, flat.n_nodes, 1), dtype=np.uint64)
    top, tips, internal, pv = tc.collapse_host(flat, sets)
    assert (top == 0).all() and tips[0] == n and internal[0] == n - 1 and (pv == -1).all()


def test_constants_as_in_the_reference():
    assert (tc.VERTICAL, tc.HORIZONTAL, tc.TRIM) == ('VERTICAL', 'HORIZONTAL', 'TRIM')


@pytest.mark.parametrize('timing', ['HORIZONTAL', 'TRIM'])
def test_later_pajek_timings_are_refused(timing, tmp_path):
    with pytest.raises(NotImplementedError, match=timing):
        pipeline.pastml_pipeline(TREE, data=TABLE, data_sep=',', columns=['Country'], pajek=str(tmp_path / 'map.net'),
                                 pajek_timing=timing)
    assert not os.path.exists(str(tmp_path / 'map.net'))


def test_unknown_pajek_timing_is_an_error(tmp_path):
    with pytest.raises(ValueError, match='pajek_timing'):
        pipeline.pastml_pipeline(TREE, data=TABLE, data_sep=',', columns=['Country'], pajek=str(tmp_path / 'map.net'),
                                 pajek_timing='SOMETIMES')


def test_html_is_still_refused_next_to_pajek(tmp_path):
    with pytest.raises(NotImplementedError, match='html_compressed'):
        pipeline.pastml_pipeline(TREE, data=TABLE, data_sep=',', columns=['Country'], pajek=str(tmp_path / 'map.net'),
                                 html_compressed=str(tmp_path / 'map.html'))


def test_pipeline_writes_the_map_without_a_gpu(tmp_path):
    """COPY needs no device: the pipeline's wiring of pajek= end to end, against the collapse of the annotations themselves."""
    from pastml_amd.acr import COPY
    out = str(tmp_path / 'map.net')
    pipeline.pastml_pipeline(TREE, data=TABLE, data_sep=',', columns=['Country'], prediction_method=COPY,
                             work_dir=str(tmp_path / 'work'), pajek=out)
    with open(out) as f:
        lines = f.read().split('\n')
    n_vertices = int(lines[0].split()[1])
    assert lines[0].startswith('*vertices ') and lines[n_vertices + 1] == '*arcs' and len(lines) == 2 * n_vertices + 1
    assert lines[1].startswith('1 "') and all('"Country:' in line for line in lines[1:n_vertices + 1])
    tips = [t for line in lines[1:n_vertices + 1] for t in line.split('"')[3].split(';') if t]
    n_tips = len(read_tree(TREE))
    assert len(tips) == n_tips and len(set(tips)) == n_tips


def test_one_large_vertex_is_written_in_linear_time():
    """
    2 * 10^5 tips in one state: one vertex holds them all, and its tip text is one join, not a fold that copies the text so
    far for every tip (a quadratic cost: minutes at this size).
    """
    n_tips = 200000
    N = n_tips + 1
    parent = np.zeros(N, dtype=np.int32)
    parent[0] = -1
    n_children = np.zeros(N, dtype=np.int32)
    n_children[0] = n_tips
    flat = FlatForest(parent, n_children, np.ones(N, dtype=np.int32), np.full(N, 0.1), np.array([0]))
    words = np.ones((N, 1), dtype=np.uint64)
    words[N - 1] = 2   # ... but the last tip: a second vertex, so that a cut is exercised
    sets = words[None]
    compressed = tc.compact(flat, *tc.collapse_host(flat, sets), columns=['col'], states=[np.array(['A', 'B'])], words=[words])
    vertices, arcs = tc.pajek_lines(compressed)
    assert len(vertices) == 2 and arcs == ['1 2 1']
    assert vertices[0] == '1 "n0" "{}" "col:A"'.format(';'.join('n{}'.format(i) for i in range(1, n_tips)))
    assert vertices[1] == '2 "n{0}" "n{0}" "col:B"'.format(n_tips)
