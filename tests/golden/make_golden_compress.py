#!/usr/bin/env python3
"""
Generates tests/golden/compress_vertical.npz by running the REAL reference's tree compressor
(pastml/visualisation/tree_compressor.py, imported unmodified through the stand-ins of make_golden.py).  Run as:

    python3 -B tests/golden/make_golden_compress.py

Per tree of a case the reference's ``compress_tree(tree, columns, pajek=[vertices, arcs], pajek_timing=VERTICAL,
tip_size_threshold=10**9)`` is called with one pair of lists for the whole forest, as ``visualize`` does
(cytoscape_manager.py:801-807); the threshold keeps its later trimming away.  The Pajek lines are taken where the reference
forms them; ``len(TIPS_INSIDE)`` and ``len(INTERNAL_NODES_INSIDE)`` of every vertex are read at the same point, through a
wrapper put in place of the module attribute ``_tree2pajek_vertices_arcs`` (the reference's files stay untouched).

The reference copies onto its compressed tree only the features that the ROOT carries (``copy_forest(..., features=columns |
set(tree.features))``), so a tree whose root has no ``polytomy`` feature loses the flag of every node and counts its
polytomy nodes among INTERNAL_NODES_INSIDE.  Case (e) gives the root ``polytomy = 0`` so that the flags are seen, which is
the behaviour line :94 is written for.

Stored per case <c>: ``<c>_newick`` (the trees, names and all), ``<c>_columns``, per column i ``<c>_states_<i>`` and
``<c>_words_<i>`` (uint64[N, W_i], FlatForest level order; all-zero: the node has no such feature), ``<c>_polytomy`` bool[N],
``<c>_vertices`` / ``<c>_arcs`` (the reference's lines), ``<c>_tips_inside`` / ``<c>_internal_inside`` (per vertex, Pajek order).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np

import make_golden  # noqa: F401  (installs the stand-ins and puts the reference on the path)
from pastml.visualisation import tree_compressor as rtc  # noqa: E402

from pastml_amd import tree as our_tree  # noqa: E402
from pastml_amd.batch import one_hot_words, n_words  # noqa: E402

assert rtc.__file__.startswith(make_golden.REF)


def reference_pajek(roots, columns):
    """(vertex lines, arc lines, tips inside, internal nodes inside) of the reference for a forest with features set."""
    vertices, arcs, n_tips, n_internal = [], [], [], []
    original = rtc._tree2pajek_vertices_arcs

    def recording(compressed_tree, nodes, edges, columns):
        for n in compressed_tree.traverse('preorder'):
            n_tips.append(len(getattr(n, rtc.TIPS_INSIDE)))
            n_internal.append(len(getattr(n, rtc.INTERNAL_NODES_INSIDE)))
        return original(compressed_tree, nodes, edges, columns=columns)

    rtc._tree2pajek_vertices_arcs = recording
    try:
        for tree in roots:
            rtc.compress_tree(tree, columns=set(columns), pajek=[vertices, arcs], pajek_timing=rtc.VERTICAL,
                              tip_size_threshold=10 ** 9)
    finally:
        rtc._tree2pajek_vertices_arcs = original
    return vertices, arcs, n_tips, n_internal


def walk_states(flat, k, rng, p_change=0.05, p_two=0.0, p_none=0.0):
    """
    State sets by a slow random walk down the tree: a node keeps its parent's set with probability 1 - p_change, else it
    draws a new state; then some nodes get a second state and some lose the feature.  uint64[N, W].
    """
    N = flat.n_nodes
    state = np.zeros(N, dtype=np.int64)
    for i in range(N):
        p = flat.parent[i]
        state[i] = rng.integers(k) if p < 0 or rng.random() < p_change else state[p]
    words = one_hot_words(state, k)
    second = np.flatnonzero(rng.random(N) < p_two)
    words[second] |= one_hot_words(rng.integers(k, size=len(second)), k)
    words[rng.random(N) < p_none] = 0
    return words


def set_features(flat, columns, states, words):
    for c, s, w in zip(columns, states, words):
        s = np.asarray(s)
        for i, node in enumerate(flat.nodes):
            bits = np.unpackbits(np.ascontiguousarray(w[i]).view(np.uint8), bitorder='little')[:len(s)].astype(bool)
            if bits.any():
                node.add_feature(c, set(s[bits].tolist()))


def state_names(k, prefix):
    return np.array(['{}{:03d}'.format(prefix, i) for i in range(k)])


def store(out, case, roots, columns, states, words, polytomy=None):
    flat = our_tree.FlatForest.from_trees(roots)
    vertices, arcs, n_tips, n_internal = reference_pajek(roots, columns)
    out[case + '_newick'] = np.array('\n'.join(r.write() for r in roots))
    out[case + '_columns'] = np.array(columns)
    for i, (s, w) in enumerate(zip(states, words)):
        out['{}_states_{}'.format(case, i)] = np.asarray(s)
        out['{}_words_{}'.format(case, i)] = np.asarray(w, dtype=np.uint64)
    out[case + '_polytomy'] = np.zeros(flat.n_nodes, dtype=bool) if polytomy is None else np.asarray(polytomy, dtype=bool)
    out[case + '_vertices'] = np.array(vertices)
    out[case + '_arcs'] = np.array(arcs)
    out[case + '_tips_inside'] = np.array(n_tips, dtype=np.int64)
    out[case + '_internal_inside'] = np.array(n_internal, dtype=np.int64)
    print('{}: {} nodes, {} vertices, largest vertex {} tips'.format(case, flat.n_nodes, len(vertices), max(n_tips)))


def case_toy(out):
    roots = [our_tree.TreeNode('((a:1,b:1,(c:1,d:0)x:1)n1:1,(e:1,(f:1,g:1)n3:0.5)n2:1,h:2)root;')]
    flat = our_tree.FlatForest.from_trees(roots)
    col = {n: {'A'} for n in 'a b d g h n1 root'.split()}
    col.update({n: {'B'} for n in 'c e f n3 n2'.split()})
    col['x'] = {'A', 'B'}
    states = [np.array(['A', 'B']), np.array(['X'])]
    words = [np.zeros((flat.n_nodes, 1), dtype=np.uint64), np.ones((flat.n_nodes, 1), dtype=np.uint64)]
    for i, node in enumerate(flat.nodes):
        words[0][i, 0] = sum(1 << j for j, s in enumerate('AB') if s in col[node.name])
    set_features(flat, ['col', 'c2'], states, words)
    store(out, 'toy', roots, ['col', 'c2'], states, words)


def random_case(out, case, n_tips, ks, seed, n_trees=1, max_arity=4, p_two=0.02, p_none=0.01):
    rng = np.random.default_rng(seed)
    flat = our_tree.FlatForest.random(n_tips, seed=seed, max_arity=max_arity, zero_frac=0.1, n_trees=n_trees)
    roots = [flat.nodes[r] for r in flat.roots]
    columns = ['char{}'.format(i) for i in range(len(ks))]
    states = [state_names(k, 's') for k in ks]
    words = [walk_states(flat, k, rng, p_two=p_two, p_none=p_none) for k in ks]
    set_features(flat, columns, states, words)
    store(out, case, roots, columns, states, words)


def case_last_word(out):
    """k = 130 (W = 3) next to a narrower column: two nodes differ from their parents ONLY in the last word of the last column."""
    rng = np.random.default_rng(130)
    flat = our_tree.FlatForest.random(60, seed=130, max_arity=3)
    roots = [flat.nodes[r] for r in flat.roots]
    columns = ['a_narrow', 'b_wide']
    states = [state_names(5, 'n'), state_names(130, 'w')]
    words = [walk_states(flat, 5, rng, p_change=0.05), np.zeros((flat.n_nodes, n_words(130)), dtype=np.uint64)]
    words[1][:, 0] = 1   # everybody has state 0 of the wide column
    internal = np.flatnonzero((flat.n_children > 0) & (flat.parent >= 0))
    tips = np.flatnonzero(flat.n_children == 0)
    for i in (internal[len(internal) // 2], tips[len(tips) // 3]):
        # ... and these two also state 129, the second bit of the third word, with the narrow column as their parent's
        words[1][i, 2] = 2
        words[0][i] = words[0][flat.parent[i]]
    set_features(flat, columns, states, words)
    store(out, 'last_word', roots, columns, states, words)


def case_resolved(out):
    """A tree after resolve_trees: IS_POLYTOMY nodes exist, and the reference leaves them out of INTERNAL_NODES_INSIDE."""
    rng = np.random.default_rng(77)
    flat = our_tree.FlatForest.random(120, seed=77, max_arity=6)
    roots = [flat.nodes[r] for r in flat.roots]
    columns = ['char0', 'char1']
    states = [state_names(3, 's'), state_names(4, 't')]
    set_features(flat, columns, states, [walk_states(flat, 3, rng, p_change=0.5), walk_states(flat, 4, rng, p_change=0.1)])
    created = our_tree.resolve_trees({c: s for c, s in zip(columns, states)}, roots)
    assert created > 0
    flat = our_tree.get_flat_forest(roots)
    from pastml_amd.batch import annotation_words
    words = [annotation_words(flat, c, s)[0] for c, s in zip(columns, states)]
    polytomy = our_tree._polytomy_flags(flat)
    assert polytomy.sum() == created
    roots[0].add_feature(our_tree.IS_POLYTOMY, 0)   # (see the module docstring: the reference copies the root's features only)
    store(out, 'resolved', roots, columns, states, words, polytomy)


def main():
    out = {}
    case_toy(out)
    random_case(out, 'ragged', 300, (4, 20, 70), seed=11)
    random_case(out, 'forest', 80, (3, 6), seed=5, n_trees=2, max_arity=3)
    case_last_word(out)
    case_resolved(out)
    np.savez_compressed(os.path.join(HERE, 'compress_vertical.npz'), **out)


if __name__ == '__main__':
    main()
