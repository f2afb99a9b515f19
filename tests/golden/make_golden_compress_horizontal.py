#!/usr/bin/env python3
"""
Generates tests/golden/compress_horizontal.npz by running the REAL reference's tree compressor
(pastml/visualisation/tree_compressor.py, imported unmodified through the stand-ins of make_golden.py).  Run as:

    python3 -B tests/golden/make_golden_compress_horizontal.py

Per tree of a case the reference's ``compress_tree(tree, columns, pajek=[vertices, arcs], pajek_timing=HORIZONTAL,
tip_size_threshold=...)`` is called with one pair of lists for the whole forest.  ``compress_tree`` goes on to trim after it
has recorded the lines of this timing; the lists are filled by then, so what is stored is unaffected (the trimming edits the
tree it is given, which is why the newick is written first).  Wrappers put in place of the module attributes
``_tree2pajek_vertices_arcs`` and ``collapse_horizontally`` (the reference's files stay untouched) read ``len(ROOTS)`` of every
vertex where the lines are formed, and the ROOTS lists before and after each pass, from which the properties that every
case is there for are ASSERTED below: inputs on which the reference merges nothing would prove nothing.

Every node is uniquely named: the reference caches configurations by node name.

Stored per case <c>: ``<c>_newick``, ``<c>_columns``, ``<c>_states_<i>``, ``<c>_words_<i>``, ``<c>_polytomy`` as in
compress_vertical.npz; ``<c>_vertices`` / ``<c>_arcs`` (the reference's lines), ``<c>_widths`` (len(ROOTS) per vertex, Pajek
order), ``<c>_threshold`` (tip_size_threshold), ``<c>_passes`` (calls of collapse_horizontally per tree before the lines).
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np

import make_golden  # noqa: F401  (installs the stand-ins and puts the reference on the path)
from pastml.visualisation import tree_compressor as rtc  # noqa: E402

from make_golden_compress import set_features, state_names, walk_states  # noqa: E402
from pastml_amd import tree as our_tree  # noqa: E402
from pastml_amd.batch import one_hot_words  # noqa: E402

assert rtc.__file__.startswith(make_golden.REF)


def reference_pajek(roots, columns, threshold):
    """(vertex lines, arc lines, widths, per tree and pass {survivor name: (ROOTS names before, after)}, per tree and pass
    the ROOTS names of every vertex before it)."""
    vertices, arcs, widths, passes, befores = [], [], [], [], []
    tree2pajek, collapse = rtc._tree2pajek_vertices_arcs, rtc.collapse_horizontally
    state = {}

    def recording_lines(compressed_tree, nodes, edges, columns):
        for n in compressed_tree.traverse('preorder'):
            widths.append(len(getattr(n, rtc.ROOTS)))
        state['recorded'] = True
        return tree2pajek(compressed_tree, nodes, edges, columns=columns)

    def recording_pass(tree, columns, tips2bin, mixed=False):
        before = {n.name: [r.name for r in getattr(n, rtc.ROOTS)] for n in tree.traverse()}
        collapse(tree, columns, tips2bin, mixed=mixed)
        if not state['recorded']:
            after = {n.name: [r.name for r in getattr(n, rtc.ROOTS)] for n in tree.traverse()}
            state['passes'].append({name: (before[name], roots) for name, roots in after.items() if roots != before[name]})
            state['before'].append(before)

    rtc._tree2pajek_vertices_arcs, rtc.collapse_horizontally = recording_lines, recording_pass
    try:
        for tree in roots:
            state.update(recorded=False, passes=[], before=[])
            for tip in tree:   # (as the reference's pipeline marks its tips; the trimming that follows the lines asks for it)
                tip.add_feature(rtc.IS_TIP, True)
            rtc.compress_tree(tree, columns=set(columns), pajek=[vertices, arcs], pajek_timing=rtc.HORIZONTAL,
                              tip_size_threshold=threshold)
            assert state['recorded']
            passes.append(state['passes'])
            befores.append(state['before'])
    finally:
        rtc._tree2pajek_vertices_arcs, rtc.collapse_horizontally = tree2pajek, collapse
    return vertices, arcs, widths, passes, befores


def store(out, case, roots, columns, states, words, threshold=rtc.REASONABLE_NUMBER_OF_TIPS):
    flat = our_tree.FlatForest.from_trees(roots)
    names = [n.name for n in flat.nodes]
    assert len(set(names)) == len(names) and all(names), 'every node needs a name of its own'
    out[case + '_newick'] = np.array('\n'.join(r.write() for r in roots))   # (before the reference trims the trees)
    vertices, arcs, widths, passes, befores = reference_pajek(roots, columns, threshold)
    out[case + '_columns'] = np.array(columns)
    for i, (s, w) in enumerate(zip(states, words)):
        out['{}_states_{}'.format(case, i)] = np.asarray(s)
        out['{}_words_{}'.format(case, i)] = np.asarray(w, dtype=np.uint64)
    out[case + '_polytomy'] = np.zeros(flat.n_nodes, dtype=bool)
    out[case + '_vertices'] = np.array(vertices)
    out[case + '_arcs'] = np.array(arcs)
    out[case + '_widths'] = np.array(widths, dtype=np.int64)
    out[case + '_threshold'] = np.array(threshold)
    out[case + '_passes'] = np.array([len(p) for p in passes], dtype=np.int64)
    print('{}: {} nodes, {} vertices, widest {}, groups per pass {}'.format(
        case, flat.n_nodes, len(vertices), max(widths), [[len(g) for g in p] for p in passes]))
    return vertices, arcs, widths, passes, befores


def named(newick_roots):
    roots = [our_tree.TreeNode(nwk) for nwk in newick_roots]
    return roots, our_tree.FlatForest.from_trees(roots)


def words_by_name(flat, states, state_of):
    """uint64[N, 1]: the one state ``state_of(name)`` of every node."""
    index = {s: i for i, s in enumerate(states)}
    return one_hot_words(np.array([index[state_of(n.name)] for n in flat.nodes]), len(states))


def arc_weights(arcs):
    return {tuple(int(x) for x in a.split()[:2]): int(a.split()[2]) for a in arcs}


def case_toy(out):
    """Two identical cherries merge (arc weight 2); a third that differs in one tip's state does not."""
    roots, flat = named(['((a1:1,b1:1)p1:1,(a2:1,b2:1)p2:1,(a3:1,b3:1)p3:1)root;'])
    states = np.array(['A', 'B', 'C', 'P', 'R'])
    words = [words_by_name(flat, states, lambda n: {'r': 'R', 'p': 'P', 'a': 'A', 'b': 'B'}[n[0]] if n != 'b3' else 'C')]
    set_features(flat, ['col'], [states], words)
    vertices, arcs, widths, passes, befores = store(out, 'toy', roots, ['col'], [states], words)
    assert len(vertices) == 7 and sorted(widths) == [1, 1, 1, 1, 1, 1, 2] and out['toy_passes'].tolist() == [1]
    assert passes[0][0] == {'p1': (['p1'], ['p1', 'p2'])}
    assert arc_weights(arcs)[(1, 2)] == 2
    assert vertices[1].split('"')[1] == 'p1' and vertices[1].split('"')[3] == ';'      # p1 and p2 hold no tips themselves
    assert vertices[2].split('"')[3] == 'a1' and vertices[4].split('"')[1] == 'p3'     # p2's tips appear nowhere


def case_widths(out):
    """X, Y, Z: equal states, equal child classes; X's and Z's merged child has width 2, Y's width 3: only X and Z merge."""
    roots, flat = named(['((x1:1,x2:1)X:1,(y1:1,y2:1,y3:1)Y:1,(z1:1,z2:1)Z:1)root;'])
    states = np.array(['I', 'R', 'T'])
    words = [words_by_name(flat, states, lambda n: 'R' if n == 'root' else 'I' if n in 'XYZ' else 'T')]
    set_features(flat, ['col'], [states], words)
    vertices, arcs, widths, passes, befores = store(out, 'widths', roots, ['col'], [states], words)
    merged = passes[0][0]
    assert merged['x1'][1] == ['x1', 'x2'] and merged['y1'][1] == ['y1', 'y2', 'y3'] and merged['X'][1] == ['X', 'Z']
    assert 'Y' not in merged and [v.split('"')[1] for v in vertices] == ['root', 'X', 'x1', 'Y', 'y1']
    assert [a.split()[2] for a in arcs] == ['2', '2', '1', '3']
    assert vertices[2].split('"')[3] == 'x1;x2'


def joins_wide_groups(merged, before_all):
    """A group of the pass whose first vertex AND a later one already had width > 1."""
    for name, (before, after) in merged.items():
        rest = after[len(before):]
        if len(before) > 1 and rest:
            owners = [n for n, roots in before_all.items() if roots[0] == rest[0]]
            if any(len(before_all[n]) > 1 for n in owners):
                return True
    return False


def case_two_passes(out, seed):
    """A ragged random tree: pass 1 merges, pass 2 runs and merges, and pass 2 joins groups that pass 1 had made."""
    rng = np.random.default_rng(seed)
    flat = our_tree.FlatForest.random(300, seed=seed, max_arity=4, zero_frac=0.1)
    roots = [flat.nodes[r] for r in flat.roots]
    columns, ks = ['char0', 'char1'], (2, 3)
    states = [state_names(k, 's') for k in ks]
    words = [walk_states(flat, k, rng, p_change=0.3) for k in ks]
    set_features(flat, columns, states, words)
    vertices, arcs, widths, passes, befores = store(out, 'two_passes', roots, columns, states, words)
    assert len(passes[0]) == 2 and len(passes[0][0]) >= 1 and len(passes[0][1]) >= 1
    assert joins_wide_groups(passes[0][1], befores[0][1]), 'no pass-2 group joins vertices that already had width > 1'


def case_decades(out):
    """Leaf vertices of 9, 10, 99 and 100 tips in one state: in pass 2, 10 and 99 merge, 9 and 100 stay."""
    sizes = {'n9': 9, 'n10': 10, 'n99': 99, 'n100': 100}
    stars = ['({}){}:1'.format(','.join('{}t{}:1'.format(name, i) for i in range(size)), name) for name, size in sizes.items()]
    extras = ['e{}:1'.format(i) for i in range(20)]   # 20 tips in states of their own: more than 15 leaf vertices, no merges
    roots, flat = named(['({})root;'.format(','.join(stars + extras))])
    states = np.array(['R', 'S'] + ['E{:02d}'.format(i) for i in range(20)])
    words = [words_by_name(flat, states, lambda n: 'R' if n == 'root' else 'E{:02d}'.format(int(n[1:])) if n[0] == 'e' else 'S')]
    set_features(flat, ['col'], [states], words)
    vertices, arcs, widths, passes, befores = store(out, 'decades', roots, ['col'], [states], words)
    assert len(passes[0]) == 2 and passes[0][0] == {} and passes[0][1] == {'n10': (['n10'], ['n10', 'n99'])}
    assert [v.split('"')[1] for v in vertices[:4]] == ['root', 'n9', 'n10', 'n100']


def case_forest(out, seed):
    """Two trees: the first keeps at most 15 leaf vertices after pass 1 (no second pass), the second has more; ids continue."""
    small = '((a1:1,b1:1)p1:1,(a2:1,b2:1)p2:1,(a3:1,c3:1)p3:1)r0;'
    rng = np.random.default_rng(seed)
    big = our_tree.FlatForest.random(120, seed=seed, max_arity=3, zero_frac=0.1)
    for node in big.nodes:
        node.name = 'T' + node.name
    roots = [our_tree.TreeNode(small), big.nodes[big.roots[0]]]
    flat = our_tree.FlatForest.from_trees(roots)
    states = [state_names(3, 's')]
    own = {'r': 0, 'p': 1, 'a': 0, 'b': 2, 'c': 1}
    walk = walk_states(flat, 3, rng, p_change=0.3)
    words = [np.where(np.array([not n.name.startswith('T') for n in flat.nodes])[:, None],
                      one_hot_words(np.array([own.get(n.name[0], 0) for n in flat.nodes]), 3), walk)]
    set_features(flat, ['char0'], states, words)
    vertices, arcs, widths, passes, befores = store(out, 'forest', roots, ['char0'], states, words)
    assert len(passes[0]) == 1 and passes[0][0] == {'p1': (['p1'], ['p1', 'p2'])}
    assert len(passes[1]) == 2 and len(passes[1][0]) >= 1 and len(passes[1][1]) >= 1
    first_of_second = [i for i, v in enumerate(vertices) if v.split('"')[1] == roots[1].name]
    assert first_of_second == [6] and vertices[6].startswith('7 "')   # r0, p1, a1, b1, p3 (with c3), a3 come first


def case_albania(out):
    """The repository's Albania files through the pipeline with COPY (no device), read back as the command line reads them."""
    import pandas as pd
    from pastml_amd import pipeline
    from pastml_amd.acr import COPY
    from pastml_amd.annotation import preannotate_forest
    from pastml_amd.visualisation import tree_compressor as tc
    tree = os.path.join(HERE, 'data', 'Albanian.tree.152tax.tre')
    with tempfile.TemporaryDirectory() as work:
        pipeline.pastml_pipeline(tree, data=os.path.join(HERE, 'data', 'data.txt'), data_sep=',', columns=['Country'],
                                 prediction_method=COPY, work_dir=work)
        roots = our_tree.read_forest(os.path.join(work, pipeline.get_named_tree_file(tree)))
        df = pd.read_csv(os.path.join(work, pipeline.get_combined_ancestral_state_file()), sep='\t', index_col=0, header=0,
                         dtype=str, keep_default_na=False)
    df.index = df.index.map(str)
    preannotate_forest(roots, df=df)
    flat = our_tree.get_flat_forest(roots)
    states = [np.array(sorted(set(df['Country']) - {''}))]
    states, words = tc.column_words(flat, ['Country'], {'Country': states[0]})
    plain = [our_tree.TreeNode(r.write()) for r in roots]   # (plain trees for the reference: features as node attributes)
    plain_flat = our_tree.FlatForest.from_trees(plain)
    assert [n.name for n in plain_flat.nodes] == [n.name for n in flat.nodes]
    set_features(plain_flat, ['Country'], states, words)
    vertices, arcs, widths, passes, befores = store(out, 'albania', plain, ['Country'], states, words)
    # (tips of one country under the one internal vertex: five leaf vertices after pass 1, so no second pass)
    assert len(passes[0]) == 1 and len(passes[0][0]) >= 1 and max(widths) > 1


def main():
    out = {}
    case_toy(out)
    case_widths(out)
    case_two_passes(out, seed=int(os.environ.get('TWO_PASSES_SEED', 1)))
    case_decades(out)
    case_forest(out, seed=int(os.environ.get('FOREST_SEED', 8)))
    case_albania(out)
    np.savez_compressed(os.path.join(HERE, 'compress_horizontal.npz'), **out)


if __name__ == '__main__':
    main()
