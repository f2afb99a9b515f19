#!/usr/bin/env python3
"""
Generates tests/golden/compress_trim.npz by running the REAL reference's tree compressor
(pastml/visualisation/tree_compressor.py, imported unmodified through the stand-ins of make_golden.py).  Run as:

    python3 -B tests/golden/make_golden_compress_trim.py

Per tree of a case the reference's ``compress_tree(tree, columns, pajek=[vertices, arcs], pajek_timing=TRIM,
tip_size_threshold=..., can_merge_diff_sizes=...)`` is called with one pair of lists for the whole forest, the tips marked
``IS_TIP`` first (the second loop of ``remove_small_tips`` asks for it).  Wrappers put in place of the module attributes
``_tree2pajek_vertices_arcs``, ``collapse_horizontally``, ``remove_small_tips`` and ``remove_mediators`` (the reference's files
stay untouched) read ``len(ROOTS)`` where the lines are formed, the threshold out of the closure of ``to_be_removed``, the
vertices before and after the removal and the splicing, and the ROOTS lists around the pass that follows them; the property
that every case is there for is ASSERTED below.

``remove_mediators`` edits the tree while a post-order traversal of it is running.  ete3 pushes a vertex's children when it
first reaches the vertex, and so does the stand-in; the wrapper counts the visits and asserts that every vertex was visited
exactly once, or the golden would not be the reference's.

Every node is uniquely named: the reference caches configurations by node name.

A vertex whose mean number of tips per configuration is no integer exists only after the pass over decades of sizes: with
``can_merge_diff_sizes=False`` every group has one number of tips, so the mean is a float with an integer value (3.0 next to
a never-merged vertex's 3).  The case ``float_num`` is that; ``final_merge`` has 3.5 under the decade bin.

Stored per case <c>: ``<c>_newick``, ``<c>_columns``, ``<c>_states_<i>``, ``<c>_words_<i>``, ``<c>_polytomy`` as in
compress_vertical.npz; ``<c>_vertices`` / ``<c>_arcs`` (the reference's lines), ``<c>_widths`` (len(ROOTS) per vertex, Pajek
order), ``<c>_tip_size_threshold``, ``<c>_can_merge``, and per tree ``<c>_thresholds`` (NaN: not trimmed), ``<c>_removed``,
``<c>_mediators`` (counts), ``<c>_mediator_names`` (all trees, ';'-joined), ``<c>_final_groups``.
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

assert rtc.__file__.startswith(make_golden.REF)


def reference_trim(roots, columns, k, can_merge):
    """(vertex lines, arc lines, widths, per tree a dict of what the wrappers saw)."""
    vertices, arcs, widths, facts = [], [], [], []
    originals = (rtc._tree2pajek_vertices_arcs, rtc.collapse_horizontally, rtc.remove_small_tips, rtc.remove_mediators)
    tree2pajek, collapse, small_tips, mediators = originals
    state = {}

    def recording_lines(compressed_tree, nodes, edges, columns):
        for n in compressed_tree.traverse('preorder'):
            widths.append(len(getattr(n, rtc.ROOTS)))
            state['num'][n.name] = getattr(n, rtc.NUM_TIPS_INSIDE)
        return tree2pajek(compressed_tree, nodes, edges, columns=columns)

    def recording_pass(tree, columns, tips2bin, mixed=False):
        before = {n.name: [r.name for r in getattr(n, rtc.ROOTS)] for n in tree.traverse()}
        nums = {n.name: getattr(n, rtc.NUM_TIPS_INSIDE) for n in tree.traverse()}
        collapse(tree, columns, tips2bin, mixed=mixed)
        after = {n.name: [r.name for r in getattr(n, rtc.ROOTS)] for n in tree.traverse()}
        state['passes'].append({name: (before[name], roots) for name, roots in after.items() if roots != before[name]})
        state['nums'].append(nums)

    def recording_small_tips(compressed_tree, full_tree, to_be_removed):
        closure = dict(zip(to_be_removed.__code__.co_freevars, (c.cell_contents for c in to_be_removed.__closure__)))
        state['threshold'] = float(closure['threshold'])
        state['passes_before_trim'] = len(state['passes'])
        before = [n.name for n in compressed_tree.traverse()]
        small_tips(compressed_tree=compressed_tree, full_tree=full_tree, to_be_removed=to_be_removed)
        after = set(n.name for n in compressed_tree.traverse())
        state['removed'] = [name for name in before if name not in after]

    def recording_mediators(tree, columns):
        before = [n.name for n in tree.traverse()]
        visits = []
        plain = tree.traverse

        def counting(strategy='levelorder'):
            for n in plain(strategy):
                visits.append(n.name)
                yield n

        tree.traverse = counting
        try:
            mediators(tree, columns)
        finally:
            del tree.traverse
        assert sorted(visits) == sorted(before), 'remove_mediators did not visit every vertex exactly once'
        after = set(n.name for n in tree.traverse())
        state['mediators'] = [name for name in before if name not in after]

    rtc._tree2pajek_vertices_arcs, rtc.collapse_horizontally, rtc.remove_small_tips, rtc.remove_mediators = \
        recording_lines, recording_pass, recording_small_tips, recording_mediators
    try:
        for tree in roots:
            state.clear()
            state.update(passes=[], nums=[], num={}, threshold=np.nan, removed=[], mediators=[], passes_before_trim=None)
            for tip in tree:
                tip.add_feature(rtc.IS_TIP, True)
            rtc.compress_tree(tree, columns=set(columns), pajek=[vertices, arcs], pajek_timing=rtc.TRIM, tip_size_threshold=k,
                              can_merge_diff_sizes=can_merge)
            facts.append(dict(state))
    finally:
        rtc._tree2pajek_vertices_arcs, rtc.collapse_horizontally, rtc.remove_small_tips, rtc.remove_mediators = originals
    return vertices, arcs, widths, facts


def store(out, case, roots, columns, states, words, k, can_merge=True):
    flat = our_tree.FlatForest.from_trees(roots)
    names = [n.name for n in flat.nodes]
    assert len(set(names)) == len(names) and all(names), 'every node needs a name of its own'
    out[case + '_newick'] = np.array('\n'.join(r.write() for r in roots))   # (before the reference trims the trees)
    vertices, arcs, widths, facts = reference_trim(roots, columns, k, can_merge)
    out[case + '_columns'] = np.array(columns)
    for i, (s, w) in enumerate(zip(states, words)):
        out['{}_states_{}'.format(case, i)] = np.asarray(s)
        out['{}_words_{}'.format(case, i)] = np.asarray(w, dtype=np.uint64)
    out[case + '_polytomy'] = np.zeros(flat.n_nodes, dtype=bool)
    out[case + '_vertices'] = np.array(vertices)
    out[case + '_arcs'] = np.array(arcs)
    out[case + '_widths'] = np.array(widths, dtype=np.int64)
    out[case + '_tip_size_threshold'] = np.array(k)
    out[case + '_can_merge'] = np.array(bool(can_merge))
    out[case + '_thresholds'] = np.array([f['threshold'] for f in facts], dtype=np.float64)
    out[case + '_removed'] = np.array([len(f['removed']) for f in facts], dtype=np.int64)
    out[case + '_mediators'] = np.array([len(f['mediators']) for f in facts], dtype=np.int64)
    out[case + '_mediator_names'] = np.array(';'.join(name for f in facts for name in f['mediators']))
    out[case + '_final_groups'] = np.array([len(f['passes'][-1]) if f['passes_before_trim'] is not None else 0 for f in facts],
                                           dtype=np.int64)
    print('{}: {} nodes, {} vertices, thresholds {}, removed {}, mediators {}'.format(
        case, flat.n_nodes, len(vertices), out[case + '_thresholds'].tolist(), out[case + '_removed'].tolist(),
        [f['mediators'] for f in facts]))
    return vertices, arcs, widths, facts


# ---------------------------------------------------------------------------------------------------------------------
# built trees: a vertex is a node with its states, ``tips`` tips of the same states under it, and the vertices below
# ---------------------------------------------------------------------------------------------------------------------
def vertex(name, states, tips=0, children=()):
    return dict(name=name, states=set(states), tips=tips, children=list(children))


def leaf(name, states, tips=1):
    """A leaf vertex of ``tips`` tips: one tip that bears the name, or a node of the name over its tips."""
    return vertex(name, states, tips=0 if tips == 1 else tips)


def _newick(v, sets):
    sets[v['name']] = v['states']
    parts = [_newick(c, sets) for c in v['children']]
    for i in range(v['tips']):
        tip = '{}_t{}'.format(v['name'], i)
        sets[tip] = v['states']
        parts.append(tip + ':1')
    return ('({}){}:1'.format(','.join(parts), v['name'])) if parts else v['name'] + ':1'


def built(out, case, trees, k, can_merge=True):
    sets = {}
    roots = [our_tree.TreeNode(_newick(t, sets)[:-2] + ';') for t in trees]
    flat = our_tree.FlatForest.from_trees(roots)
    states = np.array(sorted(set().union(*sets.values())))
    index = {s: i for i, s in enumerate(states)}
    words = np.zeros((flat.n_nodes, 1), dtype=np.uint64)
    for i, node in enumerate(flat.nodes):
        words[i, 0] = sum(1 << index[s] for s in sets[node.name])
    set_features(flat, ['col'], [states], [words])
    return store(out, case, roots, ['col'], [states], [words], k, can_merge)


def names_of(vertices):
    return [v.split('"')[1] for v in vertices]


def case_under(out):
    """Three leaf vertices, threshold 3: at the gate, not over it -- untouched."""
    vertices, arcs, widths, facts = built(out, 'under', [vertex('r', 'A', children=[leaf('a', 'B', 5), leaf('b', 'C'), leaf('c', 'D')])], 3)
    assert np.isnan(facts[0]['threshold']) and names_of(vertices) == ['r', 'a', 'b', 'c']


def case_no_small(out):
    """Over the gate, but the smallest candidate is the threshold: untouched."""
    tree = vertex('r', 'A', children=[leaf('a', 'B', 2), leaf('b', 'C', 2), leaf('c', 'D', 2), leaf('d', 'E', 2)])
    vertices, arcs, widths, facts = built(out, 'no_small', [tree], 2)
    assert np.isnan(facts[0]['threshold']) and len(vertices) == 5 and len(facts[0]['passes']) == 2


def case_plain(out):
    tree = vertex('r', 'A', children=[leaf('a', 'B', 1), leaf('b', 'C', 5), leaf('c', 'D', 2), leaf('d', 'E', 4), leaf('e', 'F', 3)])
    vertices, arcs, widths, facts = built(out, 'plain', [tree], 3)
    assert facts[0]['threshold'] == 3 and sorted(facts[0]['removed']) == ['a', 'c'] and names_of(vertices) == ['r', 'b', 'd', 'e']


def case_cascade(out):
    """i holds no tips and only small leaves: they go, i becomes a leaf of size 0 and goes too."""
    tree = vertex('r', 'A', children=[vertex('i', 'X', children=[leaf('a', 'B'), leaf('b', 'C')]),
                                      leaf('p', 'D', 5), leaf('q', 'E', 4), leaf('s', 'F', 3)])
    vertices, arcs, widths, facts = built(out, 'cascade', [tree], 3)
    assert facts[0]['threshold'] == 3 and sorted(facts[0]['removed']) == ['a', 'b', 'i'] and names_of(vertices) == ['r', 'p', 'q', 's']


def case_kept_internal(out):
    """i holds 4 tips of its own: its small children go, i stays as a leaf."""
    tree = vertex('r', 'A', children=[vertex('i', 'X', tips=4, children=[leaf('a', 'B'), leaf('b', 'C')]),
                                      leaf('p', 'D', 5), leaf('q', 'E', 3)])
    vertices, arcs, widths, facts = built(out, 'kept_internal', [tree], 3)
    assert facts[0]['threshold'] == 3 and sorted(facts[0]['removed']) == ['a', 'b'] and names_of(vertices) == ['r', 'i', 'p', 'q']


def case_ties(out):
    """Sizes 5, 3, 3, 3, 1 and threshold 3: the comparison is strict, all three 3s stay."""
    tree = vertex('r', 'A', children=[leaf('a', 'B', 3), leaf('b', 'C', 1), leaf('c', 'D', 3), leaf('d', 'E', 5), leaf('e', 'F', 3)])
    vertices, arcs, widths, facts = built(out, 'ties', [tree], 3)
    assert facts[0]['threshold'] == 3 and facts[0]['removed'] == ['b'] and names_of(vertices) == ['r', 'a', 'c', 'd', 'e']


def case_mediator(out):
    """n {A, B} between r {A} and c {B}, its other child small: n is spliced out and c goes to the END of r's children."""
    tree = vertex('r', 'A', children=[vertex('n', 'AB', children=[leaf('c', 'B', 5), leaf('s', 'C')]),
                                      leaf('x', 'D', 4), leaf('y', 'E', 3)])
    vertices, arcs, widths, facts = built(out, 'mediator', [tree], 3)
    assert facts[0]['removed'] == ['s'] and facts[0]['mediators'] == ['n'] and names_of(vertices) == ['r', 'x', 'y', 'c']


def case_chain3(out):
    """n1 > n2 > n3 > c: n3 passes, n2 {C, D} has two states but is not c | n1, n1 passes with n2 as its child."""
    n3 = vertex('n3', 'BCD', children=[leaf('c', 'B', 5), leaf('s3', 'E')])
    n2 = vertex('n2', 'CD', children=[n3, leaf('s2', 'F')])
    n1 = vertex('n1', 'ACD', children=[leaf('s1', 'G'), n2])
    tree = vertex('r', 'A', children=[n1, leaf('x', 'H', 4), leaf('y', 'I', 3)])
    vertices, arcs, widths, facts = built(out, 'chain3', [tree], 3)
    assert sorted(facts[0]['removed']) == ['s1', 's2', 's3'] and sorted(facts[0]['mediators']) == ['n1', 'n3']
    assert names_of(vertices) == ['r', 'x', 'y', 'n2', 'c'] and arcs == ['1 2 1', '1 3 1', '1 4 1', '4 5 1']


def case_order(out):
    """r's children m1 (spliced), K (kept), m2 (spliced): afterwards K, c1, c2 -- the replacements behind what stayed."""
    tree = vertex('r', 'A', children=[vertex('m1', 'AB', children=[leaf('s1', 'F'), leaf('c1', 'B', 5)]),
                                      leaf('K', 'C', 3),
                                      vertex('m2', 'AD', children=[leaf('c2', 'D', 4), leaf('s2', 'G')])])
    vertices, arcs, widths, facts = built(out, 'order', [tree], 3)
    assert sorted(facts[0]['mediators']) == ['m1', 'm2'] and names_of(vertices) == ['r', 'K', 'c1', 'c2']


def case_barred(out):
    """nT holds a tip (T > 0); na and nb merge into one vertex of width 2 (METACHILD): both stay, all else of a mediator given.
    (cT is in another decade of sizes than ca, or the pass after the trimming would merge nT and na.)"""
    def twin(x):
        return vertex('n' + x, 'AB', children=[leaf('c' + x, 'B', 5), leaf('s' + x, 'C')])
    tree = vertex('r', 'A', children=[vertex('nT', 'AB', tips=1, children=[leaf('cT', 'B', 12), leaf('sT', 'F')]),
                                      twin('a'), twin('b'), leaf('x', 'D', 4), leaf('y', 'E', 3)])
    vertices, arcs, widths, facts = built(out, 'barred', [tree], 4)
    assert facts[0]['threshold'] == 3 and sorted(facts[0]['removed']) == ['sT', 'sa'] and facts[0]['mediators'] == []
    assert names_of(vertices) == ['r', 'nT', 'cT', 'na', 'ca', 'x', 'y'] and '1 4 2' in arcs


def case_float_num(out):
    """can_merge_diff_sizes=False: X1 ~ X2 merge (num 3.0, a float), Y holds 3 tips (an int); once the small child of X is gone,
    the pass after the trimming -- still with the identity as its bin -- merges X and Y."""
    tree = vertex('r', 'A', children=[vertex('X1', 'C', tips=3, children=[leaf('s1', 'D')]),
                                      vertex('X2', 'C', tips=3, children=[leaf('s2', 'D')]),
                                      leaf('Y', 'C', 3), leaf('p', 'E', 5), leaf('q', 'F', 4), leaf('z', 'H')])
    vertices, arcs, widths, facts = built(out, 'float_num', [tree], 4, can_merge=False)
    f = facts[0]
    assert f['threshold'] == 3 and sorted(f['removed']) == ['s1', 'z'] and f['passes_before_trim'] == 1 and len(f['passes']) == 2
    assert isinstance(f['nums'][-1]['X1'], float) and isinstance(f['nums'][-1]['Y'], int)
    assert f['passes'][-1] == {'X1': (['X1', 'X2'], ['X1', 'X2', 'Y'])} and names_of(vertices) == ['r', 'X1', 'p', 'q']


def case_final_merge(out):
    """The decade pass merges X1 (3 tips) and X2 (4): num 3.5.  After the trimming X equals Y (5 tips) and the last pass merges."""
    tree = vertex('r', 'A', children=[vertex('X1', 'C', tips=3, children=[leaf('s1', 'D')]),
                                      vertex('X2', 'C', tips=4, children=[leaf('s2', 'D')]),
                                      leaf('Y', 'C', 5), leaf('p', 'E', 6), leaf('q', 'F', 4), leaf('z', 'H')])
    vertices, arcs, widths, facts = built(out, 'final_merge', [tree], 4)
    f = facts[0]
    assert f['passes_before_trim'] == 2 and f['nums'][-1]['X1'] == 3.5 and f['threshold'] == 4
    assert f['passes'][-1] == {'X1': (['X1', 'X2'], ['X1', 'X2', 'Y'])} and f['num']['X1'] == 4.0
    assert sorted(f['removed']) == ['s1', 'z'] and names_of(vertices) == ['r', 'X1', 'p', 'q']


def case_forest(out):
    """A trimmed tree, then one at the gate: the ids continue behind what the trimming left."""
    first = vertex('r', 'A', children=[leaf('a', 'B', 1), leaf('b', 'C', 5), leaf('c', 'D', 2), leaf('d', 'E', 4), leaf('e', 'F', 3)])
    second = vertex('R2', 'A', children=[leaf('a2', 'B', 5), leaf('b2', 'C'), leaf('c2', 'D')])
    vertices, arcs, widths, facts = built(out, 'forest', [first, second], 3)
    assert facts[0]['threshold'] == 3 and np.isnan(facts[1]['threshold'])
    assert names_of(vertices) == ['r', 'b', 'd', 'e', 'R2', 'a2', 'b2', 'c2'] and arcs[-1] == '5 8 1'


def case_ragged(out, seed):
    """A ragged random tree with unresolved states: both passes, a removal with a cascade, whatever mediators there are."""
    rng = np.random.default_rng(seed)
    flat = our_tree.FlatForest.random(300, seed=seed, max_arity=4, zero_frac=0.1)
    roots = [flat.nodes[r] for r in flat.roots]
    columns, ks = ['char0', 'char1'], (2, 3)
    states = [state_names(k, 's') for k in ks]
    words = [walk_states(flat, k, rng, p_change=0.3, p_two=0.2) for k in ks]
    set_features(flat, columns, states, words)
    vertices, arcs, widths, facts = store(out, 'ragged', roots, columns, states, words, 8)
    assert not np.isnan(facts[0]['threshold']) and len(facts[0]['removed']) > 20 and facts[0]['passes_before_trim'] == 2


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
    vertices, arcs, widths, facts = store(out, 'albania', plain, ['Country'], states, words, 3)
    assert not np.isnan(facts[0]['threshold']) and len(facts[0]['removed']) >= 1


def main():
    out = {}
    case_under(out)
    case_no_small(out)
    case_plain(out)
    case_cascade(out)
    case_kept_internal(out)
    case_ties(out)
    case_mediator(out)
    case_chain3(out)
    case_order(out)
    case_barred(out)
    case_float_num(out)
    case_final_merge(out)
    case_forest(out)
    case_ragged(out, seed=int(os.environ.get('RAGGED_SEED', 1)))
    case_albania(out)
    np.savez_compressed(os.path.join(HERE, 'compress_trim.npz'), **out)


if __name__ == '__main__':
    main()
