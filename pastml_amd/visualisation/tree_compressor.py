"""
The compressed tree of a reconstruction: the vertical step (pastml/visualisation/tree_compressor.py: ``collapse_vertically``
:251-298 on the lists ``compress_tree`` :87-96 starts from), the horizontal step (``collapse_horizontally`` :164-211, the two
calls of ``compress_tree`` :102-116) and the Pajek network (``_tree2pajek_vertices_arcs`` :34-51, ``save_to_pajek`` :54-80) --
what the reference writes at ``pajek_timing='VERTICAL'`` (its default), ``'HORIZONTAL'`` and ``'TRIM'``.

Every connected region of the forest whose nodes carry the same state sets in ALL columns becomes one vertex; the arcs
between vertices are the state changes.  As arrays: node n is *merged* iff it has a parent and its sets equal the parent's
in every column (a missing feature is the empty set); ``top[n]`` is n for a node that is not merged, else ``top[parent[n]]``;
a vertex is the set of nodes with one ``top`` and takes the name and states of that node.  The merged flags, ``top`` (by
pointer jumping: ceil(log2(depth)) rounds, a caterpillar is no worse than a balanced tree) and the per-vertex counts are one
call into the HIP library (``Engine.compress_vertical``); ``device=False`` restates them in numpy.  The compaction to
vertices, the order of a vertex's children and the tip lists are array passes on the host.

Order of a vertex's children (it fixes the Pajek ids).  The reference merges in post-order and appends a merged child's
final children BEHIND the children that stay, so a vertex's children come in the order of visiting its member nodes in
pre-order and emitting each member's non-member children: vertex v sorts among its siblings by
``(pre[parent[top_v]], pre[top_v])``.

Horizontal merging folds equal sibling configurations into one vertex with a width.  It is a bottom-up canonical labelling
of subtrees: the class of a vertex is (bin, its states in all columns, the set of (width, class) of its surviving children),
and among the children of a vertex those of one class collapse into the first.  One pass is one call into the HIP library
(``Engine.compress_horizontal``: exact hash-consing in a device table, level by level); ``horizontal_pass_host`` restates it
with ``np.unique`` / ``np.lexsort``.  The reference keys its cache of configurations by node NAME and so conflates vertices
with duplicate or empty names; here the key is the vertex itself.

Trimming (``compress_tree`` :118-159, ``remove_small_tips`` :214-248, ``remove_mediators`` :301-340) works on the live
vertices of the merged forest in Pajek pre-order.  The size of a vertex is its mean number of tips per configuration times the
product of the widths from the root down (float64, the reference's operations in its order); the threshold of a tree is the
``tip_size_threshold``-th largest size among the vertices larger than all their children.  The repeated removal of small leaves
is a closed form -- a vertex survives iff it is a root or its subtree, a run of the pre-order, holds a vertex of the size: a
prefix count -- and the mediators form chains that are decided from the bottom upwards.  Sizes, flags and new parents are one
call into the HIP library (``Engine.compress_trim``), restated by ``trim_host``; the child order after splicing (the children
that stayed, then the replacements), the new pre-order and the member lists are array passes on the host, and the pass after
the trimming is ``Engine.compress_horizontal`` as it is.  ``compress_tree`` is the whole compressor for all three timings.
``compress_forest(timing='TRIM')`` and ``--pajek_timing TRIM`` still raise NotImplementedError (they point to ``compress_tree``
and ``--trim``).  Sizes of 2^53 and more are an error on both paths: Python's unbounded integers are not reproduced.

Focus / mixed mode (the rest of ``compress_tree``) is not implemented.

    python -m pastml_amd.visualisation.tree_compressor --tree NAMED_TREE --states COMBINED_TABLE --pajek OUT
           [--columns ...] [--pajek_timing VERTICAL|HORIZONTAL | --trim] [--tip_size_threshold N]
           [--timeline OUT [--root_date D [D ...]] [--timeline_type SAMPLED|NODES|LTT]]

The timeline of the map -- dates, milestones and what every vertex holds at each of them -- is ``visualisation/timeline.py``.
"""
import logging

import numpy as np

VERTICAL = 'VERTICAL'
HORIZONTAL = 'HORIZONTAL'
TRIM = 'TRIM'

MAX_DEVICE_WORDS = 8   # pml_compress_vertical: sets of at most 512 states


class CompressedForest(object):
    """
    The vertically compressed forest, one row per vertex (rows in ascending ``top``):

        top                int64[V]   the vertex's first node (its name and states are the vertex's)
        name               object[V]
        tree               int64[V]   index of the tree in the forest
        parent             int64[V]   row of the vertex above, -1 for a root
        n_tips_inside      int64[V]   tips among the vertex's nodes
        n_internal_inside  int64[V]   internal nodes among them, IS_POLYTOMY nodes not counted
        order              int64[V]   rank in the pre-order of the compressed forest, trees in turn (= Pajek id - 1)
        vertex_of_node     int64[N]   row of every node's vertex
        tips, tip_offsets             the tips of the forest sorted by (order of their vertex, left-to-right leaf order):
                                      node ids, and int64[V + 1] where the vertex of each pre-order RANK begins in them
        columns, states, words        the columns of the collapse, their state lists and the packed sets [V, W_c] of the tops
    """

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @property
    def n_vertices(self):
        return len(self.top)


def _flat_of(forest):
    from pastml_amd.tree import FlatForest, get_flat_forest
    return forest if isinstance(forest, FlatForest) else get_flat_forest(forest)


def _column_states(flat, column, column2states):
    from pastml_amd.tree import StateSetColumn
    if column2states is not None and column in column2states:
        return np.asarray(column2states[column])
    col = flat.columns.get(column)
    if isinstance(col, StateSetColumn):
        return np.asarray(col.states)
    states = set()
    if flat.nodes is not None:
        for node in flat.nodes:
            value = getattr(node, column, None)
            if value:
                states |= set(value)
    return np.array(sorted(states))


def column_words(flat, columns, column2states=None):
    """(states per column, words per column uint64[N, W_c]) of the node columns, read as ``_Predictions`` reads them."""
    from pastml_amd.batch import annotation_words
    states = [_column_states(flat, c, column2states) for c in columns]
    words = [annotation_words(flat, c, s)[0] if len(s) else np.zeros((flat.n_nodes, 1), dtype=np.uint64)
             for c, s in zip(columns, states)]
    return states, words


def stacked_sets(words, n_nodes):
    """uint64 [n_cols, N, W]: the columns' words side by side, narrower ones zero-padded (the layout of the library)."""
    W = max([w.shape[1] for w in words] + [1])
    sets = np.zeros((max(1, len(words)), n_nodes, W), dtype=np.uint64)
    for i, w in enumerate(words):
        sets[i, :, :w.shape[1]] = w
    return sets


def jump_rounds(deepest):
    """Rounds of pointer jumping after which every node has looked ``deepest`` nodes up: 2^rounds >= deepest."""
    rounds = 0
    while (1 << rounds) < deepest:
        rounds += 1
    return rounds


def collapse_host(flat, sets, is_polytomy=None):
    """
    The numpy restatement of pml_compress_vertical: (top, tips_inside, internal_inside, parent_vertex), int32[N] each, the
    last three filled at the first nodes of the vertices (0 / -1 elsewhere).
    """
    N = flat.n_nodes
    ids = np.arange(N, dtype=np.int64)
    parent = flat.parent.astype(np.int64)
    has_parent = parent >= 0
    above = np.where(has_parent, parent, ids)
    merged = has_parent.copy()
    for column in sets:
        merged &= (column == column[above]).all(axis=1)
    top = np.where(merged, parent, ids)
    for _ in range(jump_rounds(flat.n_td_levels - 1)):
        top = top[top]
    is_tip = flat.n_children == 0
    counted = ~is_tip if is_polytomy is None else ~is_tip & ~np.asarray(is_polytomy, dtype=bool)
    tips_inside = np.bincount(top[is_tip], minlength=N)
    internal_inside = np.bincount(top[counted], minlength=N)
    parent_vertex = np.where((top == ids) & has_parent, top[above], -1)
    return top.astype(np.int32), tips_inside.astype(np.int32), internal_inside.astype(np.int32), parent_vertex.astype(np.int32)


def _device_ready():
    from pastml_amd import hip
    try:
        return hip.device_count() > 0
    except (hip.HipUnavailableError, OSError):
        return False


def collapse_arrays(flat, sets, is_polytomy=None, device=None, engine=None, tune=None):
    """
    (top, tips_inside, internal_inside, parent_vertex) of ``collapse_host``, from the device unless ``device`` is False (or
    None and there is none, or the sets are wider than the library takes).  device: True or a device index insists on it.
    engine: a context that holds this forest (whatever its columns); without one a tree-only context is made for the call.
    """
    from pastml_amd import hip
    fits = sets.shape[2] <= MAX_DEVICE_WORDS
    if device is None and engine is None:
        device = fits and _device_ready()
        if not fits:
            logging.getLogger('pastml').debug('Vertical collapse on the host: sets of {} words, the device path takes at most {}.'
                                              .format(sets.shape[2], MAX_DEVICE_WORDS))
    if device is False and engine is None:
        return collapse_host(flat, sets, is_polytomy)
    if not fits:
        raise ValueError('sets of {} words: the device path of the vertical collapse takes at most {} (512 states); '
                         'device=False has no bound'.format(sets.shape[2], MAX_DEVICE_WORDS))
    if engine is not None:
        return engine.compress_vertical(sets, is_polytomy)
    with hip.Engine.tree_only(flat, device=None if device is True or device is None else int(device), tune=tune) as eng:
        return eng.compress_vertical(sets, is_polytomy)


def global_preorder(flat):
    """int64[N]: rank of every node in the pre-order of the forest, trees in turn, children left to right."""
    # post_rank = pre - depth + size - 1 with the trees one after another (FlatForest._derive)
    return flat.post_rank.astype(np.int64) + flat.depth - flat.subtree_size + 1


def collapse_vertically(forest, columns, column2states=None, device=None, engine=None):
    """
    The vertical collapse of ``forest`` (TreeNode roots or a FlatForest) over ``columns``: a :class:`CompressedForest`.

    :param columns: the node columns (features) that must all agree for a node to merge into its parent
    :param column2states: column -> its states (default: those of the column as acr() left it, else the values found)
    :param device: None -- the GPU when there is one, else numpy; False -- numpy; True or an index -- the GPU, or an error
    :param engine: a hip.Engine that holds this forest, to spare the tree upload
    """
    from pastml_amd.tree import _polytomy_flags
    flat = _flat_of(forest)
    columns = list(columns)
    N = flat.n_nodes
    states, words = column_words(flat, columns, column2states)
    flags = _polytomy_flags(flat)
    top, tips_inside, internal_inside, parent_vertex = \
        collapse_arrays(flat, stacked_sets(words, N), flags if flags.any() else None, device=device, engine=engine)
    return compact(flat, top, tips_inside, internal_inside, parent_vertex, columns, states, words)


def compact(flat, top, tips_inside, internal_inside, parent_vertex, columns=(), states=(), words=()):
    """The per-node arrays of the collapse -> a :class:`CompressedForest` (host, array passes only)."""
    N = flat.n_nodes
    top = np.asarray(top, dtype=np.int64)
    tops = np.flatnonzero(top == np.arange(N))
    V = len(tops)
    row_of_top = np.full(N, -1, dtype=np.int64)
    row_of_top[tops] = np.arange(V)
    vertex_of_node = row_of_top[top]
    pv = np.asarray(parent_vertex, dtype=np.int64)[tops]
    parent = np.where(pv >= 0, row_of_top[np.maximum(pv, 0)], -1)
    pre = global_preorder(flat)

    # vertices below top_v: the tops inside the subtree of top_v, a range of the pre-order
    is_top_by_pre = np.zeros(N + 1, dtype=np.int64)
    is_top_by_pre[pre[tops] + 1] = 1
    tops_before = np.cumsum(is_top_by_pre)
    size = tops_before[pre[tops] + flat.subtree_size[tops]] - tops_before[pre[tops]]

    # siblings in the reference's order; step[v] = 1 + the vertices under the siblings before v (roots: under earlier trees)
    node_parent = flat.parent.astype(np.int64)[tops]
    key_member = np.where(parent >= 0, pre[np.maximum(node_parent, 0)], 0)
    sib = np.lexsort((pre[tops], key_member, parent))
    sorted_parent = parent[sib]
    before = np.cumsum(size[sib]) - size[sib]
    group_start = np.flatnonzero(np.concatenate(([True], sorted_parent[1:] != sorted_parent[:-1]))) if V else np.zeros(0, np.int64)
    group_of = np.cumsum(np.concatenate(([0], (sorted_parent[1:] != sorted_parent[:-1]).astype(np.int64)))) if V else \
        np.zeros(0, np.int64)
    step = np.empty(V, dtype=np.int64)
    step[sib] = before - before[group_start][group_of] + (sorted_parent >= 0)
    # order[v] = the steps of v and of every vertex above it: sums along the paths to the roots, by pointer jumping
    order = step.copy()
    above = parent.copy()
    while (above >= 0).any():
        live = above >= 0
        order[live] += order[above[live]]
        above[live] = above[above[live]]

    tips = flat.tips.astype(np.int64)
    tips = tips[np.lexsort((pre[tips], order[vertex_of_node[tips]]))]
    n_tips = np.asarray(tips_inside, dtype=np.int64)[tops]
    by_rank = np.empty(V, dtype=np.int64)
    by_rank[order] = n_tips
    tip_offsets = np.concatenate(([0], np.cumsum(by_rank)))
    names = np.array([n.name for n in flat.nodes], dtype=object)[tops] if flat.nodes is not None else \
        np.array(['n{}'.format(i) for i in tops], dtype=object)
    return CompressedForest(top=tops, name=names, tree=flat.tree_id.astype(np.int64)[tops], parent=parent, n_tips_inside=n_tips,
                            n_internal_inside=np.asarray(internal_inside, dtype=np.int64)[tops], order=order,
                            vertex_of_node=vertex_of_node, tips=tips, tip_offsets=tip_offsets, columns=list(columns),
                            states=[np.asarray(s) for s in states], words=[np.asarray(w)[tops] for w in words], flat=flat)


def _state_strings(states, words):
    """object[V]: per vertex its states joined by ' or ' in sorted order ('' for the empty set)."""
    V = len(words)
    if V == 0:
        return np.zeros(0, dtype=object)
    names = [str(s) for s in states]
    rows, inverse = np.unique(words, axis=0, return_inverse=True)
    texts = np.empty(len(rows), dtype=object)
    for i, row in enumerate(rows):
        bits = np.unpackbits(np.ascontiguousarray(row).view(np.uint8), bitorder='little')[:len(names)]
        texts[i] = ' or '.join(sorted(names[j] for j in np.flatnonzero(bits)))
    return texts[np.asarray(inverse).reshape(-1)]


def pajek_lines(compressed, columns=None):
    """
    (vertex lines, arc lines) of a :class:`CompressedForest` (below) or a :class:`HorizontalForest` (``_horizontal_lines``).

    (vertex lines, arc lines) of the reference's ``_tree2pajek_vertices_arcs`` at vertical timing, the trees of the forest
    in turn with ids that continue.  ``<tips>`` joins the tips inside by ';': at this timing the reference's TIPS_INSIDE is
    still a flat list, so its outer ';'.join runs over single tips.
    """
    if isinstance(compressed, HorizontalForest):
        return _horizontal_lines(compressed, columns)
    columns = sorted(compressed.columns if columns is None else columns)
    V = compressed.n_vertices
    by_rank = np.empty(V, dtype=np.int64)
    by_rank[compressed.order] = np.arange(V)
    flat = compressed.flat
    names = np.array([n.name for n in flat.nodes], dtype=object) if flat.nodes is not None else \
        np.array(['n{}'.format(i) for i in range(flat.n_nodes)], dtype=object)
    counts = np.diff(compressed.tip_offsets)
    tip_text = np.full(V, '', dtype=object)
    some = np.flatnonzero(counts > 0)
    if len(some):
        # the names of a vertex's tips are one run of the sorted tips: ONE join over all of them, cut at the runs' character
        # offsets (linear in the text, however many tips a vertex holds)
        tip_names = [str(x) for x in names[compressed.tips].tolist()]
        text = ';'.join(tip_names)
        ends = np.cumsum(np.fromiter((len(x) for x in tip_names), dtype=np.int64, count=len(tip_names)) + 1)   # behind each ';'
        begins = np.concatenate(([0], ends))[compressed.tip_offsets[:-1][some]]
        stops = ends[compressed.tip_offsets[1:][some] - 1] - 1
        tip_text[some] = [text[a:b] for a, b in zip(begins.tolist(), stops.tolist())]
    ids = np.array([str(i) for i in range(1, V + 1)], dtype=object)
    lines = ids + ' "' + np.array([str(x) for x in compressed.name[by_rank]], dtype=object) + '" "' + tip_text + '"'
    for c in columns:
        i = compressed.columns.index(c)
        lines = lines + ' "' + '{}:'.format(c) + _state_strings(compressed.states[i], compressed.words[i])[by_rank] + '"'
    child = np.flatnonzero(compressed.parent[by_rank] >= 0)
    up = compressed.order[compressed.parent[by_rank[child]]] + 1
    arcs = ['{} {} 1'.format(a, b) for a, b in zip(up.tolist(), (child + 1).tolist())]
    return lines.tolist() if V else [], arcs


def save_to_pajek(compressed, columns, path):
    """
    Writes the compressed forest as a Pajek network, in the layout of the reference's ``save_to_pajek``:

    *vertices <number_of_vertices>
    <id> "<vertex_name>" "<tips_inside>" "<column1>:<state(s)>" ["<column2>:<state(s)>" ...]
    ...
    *arcs
    <source_id> <target_id> <width of the target: 1 in a vertical map>
    ...

    (no newline after the last arc).  ``columns``: those to list, sorted by name; None for all of the collapse.
    """
    vertices, arcs = pajek_lines(compressed, columns)
    with open(path, 'w+') as f:
        f.write('*vertices {}\n'.format(len(vertices)))
        f.write('\n'.join(vertices))
        f.write('\n')
        f.write('*arcs\n')
        f.write('\n'.join(arcs))


# ---------------------------------------------------------------------------------------------------------------------
# horizontal merging
# ---------------------------------------------------------------------------------------------------------------------
REASONABLE_NUMBER_OF_TIPS = 15


class HorizontalForest(object):
    """
    The horizontally merged forest, one entry per LIVE vertex in Pajek (pre-)order:

        compressed         the :class:`CompressedForest` it was merged from
        vertex             int64[L]      row of the live vertex in ``compressed`` (its name and states are the entry's)
        width              int64[L]      configurations merged into it (the weight of the arc that enters it)
        parent             int64[L]      entry of the vertex above, -1 for a root
        n_tips_total       int64[L]      tips inside over all its configurations
        members            int64[M]      rows of ``compressed``, the configurations of each entry in the reference's order
        member_offsets     int64[L + 1]  where the members of each entry begin
        merged_groups      [pass 1, pass 2]  groups of two or more that each pass merged
        second_pass        bool[n_trees]     the trees that got the pass over decades of sizes
    """

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @property
    def n_vertices(self):
        return len(self.vertex)


def _rows_as_ids(rows):
    """int64[n]: equal numbers for equal rows of an integer matrix [n, m], and only for those."""
    if rows.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    if rows.shape[1] == 0:
        return np.zeros(rows.shape[0], dtype=np.int64)
    return np.asarray(np.unique(rows, axis=0, return_inverse=True)[1]).reshape(-1).astype(np.int64)


def vertex_depths(parent, live):
    """int64[V]: branches between a live vertex and its root (0 for the others), by pointer jumping."""
    depth = ((parent >= 0) & live).astype(np.int64)
    above = np.where(live, parent, -1)
    while (above >= 0).any():
        on = np.flatnonzero(above >= 0)
        depth[on] += depth[above[on]]
        above[on] = above[above[on]]
    return depth


def horizontal_pass_host(parent, rank, bins, width, live, sets):
    """
    The numpy restatement of pml_compress_horizontal: one pass over a vertex forest, (into int32[V], live bool[V],
    width int32[V], groups merged).  Level by level from the deepest vertices up; the classes of a level are rows made equal by
    ``np.unique`` (the child lists of one length at a time, as one matrix), the sibling groups one ``np.lexsort``.  No bound on W.
    """
    parent = np.asarray(parent, dtype=np.int64)
    rank = np.asarray(rank, dtype=np.int64)
    bins = np.asarray(bins, dtype=np.int64)
    live = np.asarray(live, dtype=bool)
    V = len(parent)
    w = np.asarray(width, dtype=np.int64).copy()
    sets = np.asarray(sets, dtype=np.uint64)
    depth = vertex_depths(parent, live)
    sclass = np.zeros(V, dtype=np.int64)
    sclass[live] = _rows_as_ids(np.moveaxis(sets, 0, 1).reshape(V, -1)[live].view(np.int64))
    cls = np.zeros(V, dtype=np.int64)
    stays = live.copy()               # not merged into a sibling
    into = np.arange(V, dtype=np.int64)
    groups = 0
    ids = np.flatnonzero(live)
    ids = ids[np.argsort(depth[ids], kind='stable')]
    n_levels = int(depth[ids[-1]]) + 1 if len(ids) else 0
    bounds = np.searchsorted(depth[ids], np.arange(n_levels + 1))
    pos = np.full(V, -1, dtype=np.int64)
    for d in range(n_levels - 1, -1, -1):
        L = ids[bounds[d]:bounds[d + 1]]
        below = ids[bounds[d + 1]:bounds[d + 2]] if d + 1 < n_levels else ids[:0]
        C = below[stays[below]]
        pos[L] = np.arange(len(L))
        # the children of every vertex of the level in canonical order, as numbers of their (width, class)
        o = np.lexsort((cls[C], w[C], pos[parent[C]]))
        C = C[o]
        item = _rows_as_ids(np.stack([w[C], cls[C]], axis=1))
        arity = np.bincount(pos[parent[C]], minlength=len(L))
        start = np.cumsum(arity) - arity
        child_sig = np.zeros(len(L), dtype=np.int64)
        for a in np.unique(arity):
            if a:
                sel = np.flatnonzero(arity == a)
                child_sig[sel] = _rows_as_ids(item[start[sel][:, None] + np.arange(a)[None, :]])
        cls[L] = _rows_as_ids(np.stack([bins[L], sclass[L], arity, child_sig], axis=1))
        # siblings of one class: the first in child order takes them all
        M = L[parent[L] >= 0]
        if len(M):
            M = M[np.lexsort((rank[M], cls[M], parent[M]))]
            new = np.concatenate(([True], (parent[M][1:] != parent[M][:-1]) | (cls[M][1:] != cls[M][:-1])))
            starts = np.flatnonzero(new)
            first = M[starts][np.cumsum(new) - 1]
            into[M] = first
            stays[M] = M == first
            w[M[starts]] = np.add.reduceat(w[M], starts)
            groups += int((np.diff(np.concatenate((starts, [len(M)]))) > 1).sum())
    gone = live & ~stays
    for d in range(1, n_levels):
        L = ids[bounds[d]:bounds[d + 1]]
        gone[L] |= gone[parent[L]]
    return into.astype(np.int32), live & ~gone, w.astype(np.int32), groups


def _pass_runner(compressed, sets, device, engine):
    """(function of (bins, width, live) that runs one pass, function that releases what it holds): device selection as in
    ``collapse_arrays``."""
    from pastml_amd import hip
    parent = compressed.parent.astype(np.int32)
    rank = compressed.order.astype(np.int32)
    fits = sets.shape[2] <= MAX_DEVICE_WORDS
    if device is None and engine is None:
        device = fits and _device_ready()
        if not fits:
            logging.getLogger('pastml').debug('Horizontal merging on the host: sets of {} words, the device path takes at most {}.'
                                              .format(sets.shape[2], MAX_DEVICE_WORDS))
    if device is False and engine is None:
        return (lambda bins, width, live: horizontal_pass_host(parent, rank, bins, width, live, sets)), (lambda: None)
    if not fits:
        raise ValueError('sets of {} words: the device path of the horizontal merging takes at most {} (512 states); '
                         'device=False has no bound'.format(sets.shape[2], MAX_DEVICE_WORDS))
    if engine is not None:
        return (lambda bins, width, live: engine.compress_horizontal(parent, rank, bins, width, live, sets)), (lambda: None)
    own = hip.Engine.tree_only(compressed.flat, device=None if device is True or device is None else int(device))
    return (lambda bins, width, live: own.compress_horizontal(parent, rank, bins, width, live, sets)), own.close


def collapse_horizontally(compressed, tip_size_threshold=REASONABLE_NUMBER_OF_TIPS, can_merge_diff_sizes=True, device=None,
                          engine=None):
    """
    The horizontal merging of a :class:`CompressedForest` as ``compress_tree`` :102-116 does it, every tree on its own: a pass
    with the number of tips inside as the bin, then -- for the trees that still have more than ``tip_size_threshold`` leaf
    vertices, if ``can_merge_diff_sizes`` -- a pass with the decade of the mean number of tips per configuration.  Returns a
    :class:`HorizontalForest`.  device / engine: as for ``collapse_vertically`` (the engine is used for its device and stream).
    """
    V = compressed.n_vertices
    parent = compressed.parent
    tree = compressed.tree
    n_trees = int(tree.max()) + 1 if V else 0
    sets = stacked_sets(compressed.words, V)
    run, release = _pass_runner(compressed, sets, device, engine)
    try:
        tips = compressed.n_tips_inside.astype(np.int64)
        into1, live, width, groups1 = run(tips.astype(np.int32), np.ones(V, dtype=np.int32), np.ones(V, dtype=bool))
        width = width.astype(np.int64)
        total = np.zeros(V, dtype=np.int64)
        np.add.at(total, into1, tips)
        has_live_child = np.zeros(V, dtype=bool)
        has_live_child[parent[live & (parent >= 0)]] = True
        second = np.zeros(n_trees, dtype=bool)
        if can_merge_diff_sizes:
            second = np.bincount(tree[live & ~has_live_child], minlength=n_trees) > tip_size_threshold
        into2, groups2 = np.arange(V, dtype=np.int32), 0
        live_in = live & second[tree]
        if live_in.any():
            logging.getLogger('pastml').debug('Allowed merging nodes of different sizes.')
            bins = np.log10(np.maximum(1, total / width)).astype(np.int64)   # int(np.log10(max(1, NUM_TIPS_INSIDE))) :111
            into2, live2, width2, groups2 = run(np.where(live_in, bins, 0).astype(np.int32), width.astype(np.int32), live_in)
            live = np.where(second[tree], live2, live)
            width = np.where(live_in, width2.astype(np.int64), width)
    finally:
        release()
    for groups in (groups1, groups2):
        if groups:
            logging.getLogger('pastml').debug('Collapsed {} sets of equivalent configurations horizontally.'.format(groups))

    # the configurations of a live vertex s: the vertices u under a live parent (or roots) with into2[into1[u]] == s, in the
    # order of the reference's lists: the groups of pass 1 that pass 2 joined in child order, each in child order
    order = compressed.order
    final = into2[into1].astype(np.int64)
    proper = (parent < 0) | live[np.maximum(parent, 0)]
    members = np.flatnonzero(proper)
    members = members[np.lexsort((order[members], order[into1[members]], order[final[members]]))]
    vertex = np.flatnonzero(live)
    vertex = vertex[np.argsort(order[vertex])]
    entry = np.full(V, -1, dtype=np.int64)
    entry[vertex] = np.arange(len(vertex))
    counts = np.bincount(entry[final[members]], minlength=len(vertex))
    n_tips_total = np.zeros(len(vertex), dtype=np.int64)
    np.add.at(n_tips_total, entry[final[members]], compressed.n_tips_inside[members])
    up = parent[vertex]
    return HorizontalForest(compressed=compressed, vertex=vertex, width=width[vertex],
                            parent=np.where(up >= 0, entry[np.maximum(up, 0)], -1), n_tips_total=n_tips_total, members=members,
                            member_offsets=np.concatenate(([0], np.cumsum(counts))), merged_groups=[int(groups1), int(groups2)],
                            second_pass=second)


# ---------------------------------------------------------------------------------------------------------------------
# trimming
# ---------------------------------------------------------------------------------------------------------------------
MAX_EXACT = float(2 ** 53)   # multipliers and sizes from here on are refused: float64 no longer holds every integer


class TrimmedForest(HorizontalForest):
    """
    The trimmed forest: a :class:`HorizontalForest` (``merged_groups`` has a third entry, the groups of the pass after the
    trimming) and

        threshold          float64[n_trees]  the size threshold of each tree, NaN where the tree was not trimmed
        removed            int64[]           rows of ``compressed``: the vertices that the removal of small tips took out
        mediators          int64[]           rows of ``compressed``: the mediators spliced out
        horizontal         the :class:`HorizontalForest` it was trimmed from
    """


def _check_vertex_forest(parent, tree, n_tips_total, width, n_trees):
    """(depth int64[L], subtree size int64[L]) of a vertex forest in pre-order, or a ValueError that says what is wrong."""
    L = len(parent)
    ids = np.arange(L, dtype=np.int64)
    if ((parent < -1) | (parent >= ids)).any():
        bad = int(np.flatnonzero((parent < -1) | (parent >= ids))[0])
        raise ValueError('parent[{}] = {}: the entries are in pre-order, a parent comes before its children'.format(bad, parent[bad]))
    if (width < 1).any():
        raise ValueError('width[{}] < 1'.format(int(np.flatnonzero(width < 1)[0])))
    if (n_tips_total < 0).any():
        raise ValueError('n_tips_total[{}] < 0'.format(int(np.flatnonzero(n_tips_total < 0)[0])))
    if ((tree < 0) | (tree >= n_trees)).any():
        raise ValueError('tree ids must lie in [0, {})'.format(n_trees))
    child = parent >= 0
    if (tree[child] != tree[parent[child]]).any():
        raise ValueError('a vertex and its parent are in different trees')
    depth = vertex_depths(parent, np.ones(L, dtype=bool))
    size = np.ones(L, dtype=np.int64)
    by_depth = np.argsort(depth, kind='stable')
    bounds = np.searchsorted(depth[by_depth], np.arange(int(depth.max()) + 2 if L else 1))
    for d in range(len(bounds) - 2, 0, -1):
        level = by_depth[bounds[d]:bounds[d + 1]]
        np.add.at(size, parent[level], size[level])
    if (ids[child] + size[child] > parent[child] + size[parent[child]]).any():
        raise ValueError('the entries are not in pre-order: a subtree is no run of consecutive entries')
    return depth, size


def trim_host(parent, tree, n_tips_total, width, sets, tip_size_threshold, trim_tree):
    """
    The numpy restatement of pml_compress_trim over the live vertices of a horizontally merged forest, entries in pre-order:
    parent int[L] (-1: a root, else < the entry), tree int[L], n_tips_total int[L], width int[L], sets uint64[n_cols, L, W] (no
    bound on W), trim_tree bool[n_trees] (the trees over the gate).  Returns

        tsize       float64[L]  (n_tips_total / width) * the product of the widths from the root down, 0 outside the trees to trim
        keep        bool[L]     survives the removal of small tips (True outside the trimmed trees)
        spliced     bool[L]     a mediator that is spliced out
        new_parent  int32[L]    the entry above afterwards (-1: a root, or a vertex that is gone)
        moved       bool[L]     re-attached behind the children that stayed (its parent of before was spliced out)
        threshold   float64[n_trees]  NaN where nothing happens to the tree
    """
    parent = np.asarray(parent, dtype=np.int64)
    tree = np.asarray(tree, dtype=np.int64)
    T = np.asarray(n_tips_total, dtype=np.int64)
    w = np.asarray(width, dtype=np.int64)
    sets = np.asarray(sets, dtype=np.uint64)
    trim_tree = np.asarray(trim_tree, dtype=bool)
    k = int(tip_size_threshold)
    if k < 0:
        raise ValueError('tip_size_threshold must not be negative, got {}'.format(k))
    L, n_trees = len(parent), len(trim_tree)
    depth, size = _check_vertex_forest(parent, tree, T, w, n_trees)
    ids = np.arange(L, dtype=np.int64)
    tsize = np.zeros(L, dtype=np.float64)
    keep = np.ones(L, dtype=bool)
    spliced = np.zeros(L, dtype=bool)
    moved = np.zeros(L, dtype=bool)
    new_parent = parent.astype(np.int32)
    threshold = np.full(n_trees, np.nan)
    if not trim_tree.any():
        return tsize, keep, spliced, new_parent, moved, threshold
    on = trim_tree[tree]

    # sizes: the multiplier by pointer jumping with products (exact below 2^53, whatever the order of the factors)
    mult = w.astype(np.float64)
    up = parent.copy()
    for _ in range(jump_rounds(int(depth.max()) + 1)):
        has = np.flatnonzero(up >= 0)
        mult[has], up[has] = mult[has] * mult[up[has]], up[up[has]]
    tsize = np.where(on, (T.astype(np.float64) / w.astype(np.float64)) * mult, 0.)
    if ((mult >= MAX_EXACT) & on).any() or (tsize >= MAX_EXACT).any():
        raise ValueError('the widths along a path multiply to 2^53 or more: sizes beyond the exact range of float64 are not supported')

    # threshold: the k-th largest among the non-root vertices that are larger than all their children
    child = parent >= 0
    child_max = np.zeros(L, dtype=np.float64)
    np.maximum.at(child_max, parent[child], tsize[child])
    candidate = child & on & (tsize > child_max)
    for t in np.flatnonzero(trim_tree):
        values = np.sort(tsize[candidate & (tree == t)])
        if len(values) == 0:
            continue
        chosen = values[-k] if 0 < k <= len(values) else values[0]
        if values[0] < chosen:
            threshold[t] = chosen
    trimmed = ~np.isnan(threshold)
    if not trimmed.any():
        return tsize, keep, spliced, new_parent, moved, threshold
    on = trimmed[tree]

    # removal: a vertex survives iff it is a root or its subtree -- a run of the pre-order -- holds a vertex of the size
    big = on & (tsize >= np.where(on, threshold[tree], 0.))
    before = np.concatenate(([0], np.cumsum(big)))
    keep = ~on | ~child | (before[ids + size] - before[ids] > 0)

    # mediators: chains of candidates, each the only surviving child of the one above, decided from the bottom upwards
    kept_child = np.flatnonzero(child & keep)
    n_kept = np.bincount(parent[kept_child], minlength=L)
    only = np.zeros(L, dtype=np.int64)
    only[parent[kept_child]] = kept_child
    structural = on & keep & child & (w == 1) & (T == 0) & (n_kept == 1)
    bits = np.unpackbits(np.ascontiguousarray(sets).view(np.uint8), axis=2).sum(axis=2) if sets.size else np.zeros(sets.shape[:2], int)
    front = np.flatnonzero(structural & ~structural[only])
    below = only[front]
    while len(front):
        fits = ((sets[:, front] == (sets[:, below] | sets[:, parent[front]])).all(axis=2) & (bits[:, front] >= 2)).all(axis=0)
        spliced[front] = fits
        below = np.where(fits, below, front)
        go = structural[parent[front]]
        front, below = parent[front][go], below[go]
    above = parent.copy()
    while True:
        jump = np.flatnonzero((above >= 0) & spliced[np.maximum(above, 0)])
        if not len(jump):
            break
        above[jump] = parent[above[jump]]
    stays = keep & ~spliced
    new_parent = np.where(stays, above, -1).astype(np.int32)
    moved = stays & (above != parent)
    return tsize, keep, spliced, new_parent, moved, threshold


def _engine_for(flat, n_words_wide, device, engine, what):
    """(the engine to call or None for numpy, function that releases it): device selection as in ``collapse_arrays``."""
    from pastml_amd import hip
    fits = n_words_wide <= MAX_DEVICE_WORDS
    if device is None and engine is None:
        device = fits and _device_ready()
        if not fits:
            logging.getLogger('pastml').debug('{} on the host: sets of {} words, the device path takes at most {}.'
                                              .format(what, n_words_wide, MAX_DEVICE_WORDS))
    if device is False and engine is None:
        return None, (lambda: None)
    if not fits:
        raise ValueError('sets of {} words: the device path of the {} takes at most {} (512 states); '
                         'device=False has no bound'.format(n_words_wide, what.lower(), MAX_DEVICE_WORDS))
    if engine is not None:
        return engine, (lambda: None)
    own = hip.Engine.tree_only(flat, device=None if device is True or device is None else int(device))
    return own, own.close


def _preorder_ranks(parent, size, key):
    """int64[V]: rank in the pre-order of a forest whose siblings (and roots) come in ascending ``key``; size: subtree sizes."""
    V = len(parent)
    if V == 0:
        return np.zeros(0, dtype=np.int64)
    sib = np.lexsort((key, parent))
    sorted_parent = parent[sib]
    before = np.cumsum(size[sib]) - size[sib]
    new_group = np.concatenate(([True], sorted_parent[1:] != sorted_parent[:-1]))
    step = np.empty(V, dtype=np.int64)
    step[sib] = before - before[np.flatnonzero(new_group)][np.cumsum(new_group) - 1] + (sorted_parent >= 0)
    order = step.copy()
    above = parent.copy()
    while (above >= 0).any():
        on = np.flatnonzero(above >= 0)
        order[on] += order[above[on]]
        above[on] = above[above[on]]
    return order


def trim(merged, tip_size_threshold=REASONABLE_NUMBER_OF_TIPS, can_merge_diff_sizes=True, device=None, engine=None):
    """
    The trimming of a :class:`HorizontalForest` as ``compress_tree`` :118-156 does it, every tree on its own: a tree with more
    than ``tip_size_threshold`` leaf vertices loses the vertices whose subtrees hold nothing of the size of its
    ``tip_size_threshold``-th largest tip (``remove_small_tips``), then the mediators (``remove_mediators``), then gets one more
    horizontal pass.  The sizes, the flags and the new parents are one call into the HIP library (``Engine.compress_trim``) or
    ``trim_host``; the new child order, the pre-order and the member lists are array passes on the host; the pass is
    ``Engine.compress_horizontal`` / ``horizontal_pass_host``.  Returns a :class:`TrimmedForest`.
    """
    k = int(tip_size_threshold)
    if k < 0:
        raise ValueError('tip_size_threshold must not be negative, got {}'.format(k))
    compressed = merged.compressed
    L = merged.n_vertices
    parent = merged.parent.astype(np.int64)
    tree = compressed.tree[merged.vertex]
    n_trees = len(merged.second_pass)
    has_child = np.zeros(L, dtype=bool)
    has_child[parent[parent >= 0]] = True
    over_gate = np.bincount(tree[~has_child], minlength=n_trees) > k
    sets = stacked_sets([w[merged.vertex] for w in compressed.words], L)
    if L and max(int(merged.n_tips_total.max()), int(merged.width.max())) > np.iinfo(np.int32).max:
        raise ValueError('tips or widths beyond 32 bits')
    eng, release = _engine_for(compressed.flat, sets.shape[2], device, engine, 'Trimming')
    try:
        arrays = (parent.astype(np.int32), tree.astype(np.int32), merged.n_tips_total.astype(np.int32), merged.width.astype(np.int32),
                  sets, k, over_gate)
        if not L:
            tsize, keep, spliced, new_parent, moved, threshold = (np.zeros(0), np.zeros(0, bool), np.zeros(0, bool),
                                                                  np.zeros(0, np.int32), np.zeros(0, bool), np.full(n_trees, np.nan))
        else:
            tsize, keep, spliced, new_parent, moved, threshold = (trim_host if eng is None else eng.compress_trim)(*arrays)
        trimmed = ~np.isnan(threshold)
        log = logging.getLogger('pastml')
        for t in np.flatnonzero(trimmed):
            log.debug('Set tip size threshold to {} (the size of the {}-th largest tip).'.format(threshold[t], k))

        # the forest that is left, children in the order of the reference: those that stayed, then those re-attached, each in
        # the old order (entries are in pre-order, so the order of the chain tops is the order of what replaces them)
        stays = np.flatnonzero(keep & ~spliced)
        n = len(stays)
        entry = np.full(L, -1, dtype=np.int64)
        entry[stays] = np.arange(n)
        up = new_parent[stays].astype(np.int64)
        up = np.where(up >= 0, entry[np.maximum(up, 0)], -1)
        depth, old_size = _check_vertex_forest(parent, tree.astype(np.int64), merged.n_tips_total.astype(np.int64),
                                               merged.width.astype(np.int64), n_trees) if L else (np.zeros(0, np.int64),) * 2
        stays_before = np.concatenate(([0], np.cumsum(keep & ~spliced)))
        size = stays_before[stays + old_size[stays]] - stays_before[stays]
        order = _preorder_ranks(up, size, moved[stays].astype(np.int64) * L + stays)
        by_rank = np.empty(n, dtype=np.int64)
        by_rank[order] = np.arange(n)
        old = stays[by_rank]                         # old entry of every new one, new pre-order
        up = np.where(up[by_rank] >= 0, order[np.maximum(up[by_rank], 0)], -1)
        width = merged.width[old].astype(np.int64)
        total = merged.n_tips_total[old].astype(np.int64)

        # the pass after the trimming, over the trimmed trees: the bin that was bound last
        into, live, groups = np.arange(n, dtype=np.int64), np.ones(n, dtype=bool), 0
        in_pass = trimmed[tree[old]]
        if in_pass.any():
            num = total / width
            decade = (np.asarray(merged.second_pass, dtype=bool) & bool(can_merge_diff_sizes))[tree[old]]
            bins = np.where(decade, np.log10(np.maximum(1, num)).astype(np.int64), np.unique(num, return_inverse=True)[1].reshape(-1))
            args = (up.astype(np.int32), np.arange(n, dtype=np.int32), np.where(in_pass, bins, 0).astype(np.int32),
                    width.astype(np.int32), in_pass, sets[:, old])
            into, live2, width2, groups = (horizontal_pass_host if eng is None else eng.compress_horizontal)(*args)
            into = into.astype(np.int64)
            live = np.where(in_pass, live2, True)
            width = np.where(in_pass, width2.astype(np.int64), width)
    finally:
        release()
    if groups:
        logging.getLogger('pastml').debug('Collapsed {} sets of equivalent configurations horizontally.'.format(groups))

    # members: a survivor takes the configurations of the siblings merged into it, in the new child order
    final = np.flatnonzero(live)
    row = np.full(n, -1, dtype=np.int64)
    row[final] = np.arange(len(final))
    proper = np.flatnonzero((up < 0) | live[np.maximum(up, 0)])
    proper = proper[np.lexsort((proper, row[into[proper]]))]
    begin, count = merged.member_offsets[:-1][old[proper]], np.diff(merged.member_offsets)[old[proper]]
    ends = np.cumsum(count)
    members = merged.members[np.repeat(begin - (ends - count), count) + np.arange(int(ends[-1]) if len(ends) else 0)]
    counts = np.zeros(len(final), dtype=np.int64)
    np.add.at(counts, row[into[proper]], count)
    offsets = np.concatenate(([0], np.cumsum(counts)))
    n_tips_total = np.zeros(len(final), dtype=np.int64)
    np.add.at(n_tips_total, np.repeat(np.arange(len(final)), counts), compressed.n_tips_inside[members])
    return TrimmedForest(compressed=compressed, vertex=merged.vertex[old[final]], width=width[final],
                         parent=np.where(up[final] >= 0, row[np.maximum(up[final], 0)], -1), n_tips_total=n_tips_total,
                         members=members, member_offsets=offsets, merged_groups=list(merged.merged_groups) + [int(groups)],
                         second_pass=merged.second_pass, threshold=threshold, removed=merged.vertex[~keep],
                         mediators=merged.vertex[spliced], horizontal=merged, tsize=tsize)


def _horizontal_lines(merged, columns=None):
    """
    (vertex lines, arc lines) at horizontal timing: the live vertices in pre-order; ``<tips>`` joins the configurations of a
    vertex by ';', each the names of its tips joined by ',' in the order the vertical map lists them; an arc carries the
    width of the vertex it enters.
    """
    compressed = merged.compressed
    columns = sorted(compressed.columns if columns is None else columns)
    L = merged.n_vertices
    flat = compressed.flat
    names = np.array([n.name for n in flat.nodes], dtype=object) if flat.nodes is not None else \
        np.array(['n{}'.format(i) for i in range(flat.n_nodes)], dtype=object)
    tip_names = [str(x) for x in names[compressed.tips].tolist()]
    begins = compressed.tip_offsets[compressed.order[merged.members]].tolist()
    ends = compressed.tip_offsets[compressed.order[merged.members] + 1].tolist()
    configurations = [','.join(tip_names[a:b]) for a, b in zip(begins, ends)]
    offsets = merged.member_offsets.tolist()
    tip_text = np.array([';'.join(configurations[offsets[i]:offsets[i + 1]]) for i in range(L)] + [None], dtype=object)[:L]
    ids = np.array([str(i) for i in range(1, L + 1)], dtype=object)
    lines = ids + ' "' + np.array([str(x) for x in compressed.name[merged.vertex]] + [None], dtype=object)[:L] + '" "' + tip_text + '"'
    for c in columns:
        i = compressed.columns.index(c)
        lines = lines + ' "' + '{}:'.format(c) + _state_strings(compressed.states[i], compressed.words[i][merged.vertex]) + '"'
    child = np.flatnonzero(merged.parent >= 0)
    arcs = ['{} {} {}'.format(a + 1, b + 1, w)
            for a, b, w in zip(merged.parent[child].tolist(), child.tolist(), merged.width[child].tolist())]
    return lines.tolist() if L else [], arcs


def compress_forest(forest, columns, column2states=None, timing=VERTICAL, tip_size_threshold=REASONABLE_NUMBER_OF_TIPS,
                    can_merge_diff_sizes=True, device=None, engine=None):
    """
    The compressed forest as ``compress_tree`` has it when it records the Pajek lines of ``timing``: a
    :class:`CompressedForest` for VERTICAL, a :class:`HorizontalForest` for HORIZONTAL (``pajek_lines`` / ``save_to_pajek`` take
    both).  TRIM is refused here: the trimmed forest is ``compress_tree`` (``--trim`` on the command line).
    """
    if timing == TRIM:
        raise NotImplementedError('timing={}: compress_forest stops at {} and {}; the trimmed forest is compress_tree(..., '
                                  'pajek_timing={}), --trim on the command line'.format(TRIM, VERTICAL, HORIZONTAL, TRIM))
    if timing not in (VERTICAL, HORIZONTAL):
        raise ValueError('timing must be one of {}, {} or {}, not {!r}'.format(VERTICAL, HORIZONTAL, TRIM, timing))
    compressed = collapse_vertically(forest, columns, column2states, device=device, engine=engine)
    if timing == VERTICAL:
        return compressed
    return collapse_horizontally(compressed, tip_size_threshold=tip_size_threshold, can_merge_diff_sizes=can_merge_diff_sizes,
                                 device=device, engine=engine)


def compress_tree(forest, columns, column2states=None, tip_size_threshold=REASONABLE_NUMBER_OF_TIPS, can_merge_diff_sizes=True,
                  pajek_timing=TRIM, device=None, engine=None):
    """
    The whole compressor under the reference's name: the forest as ``compress_tree`` has it when it records the Pajek lines of
    ``pajek_timing`` -- a :class:`CompressedForest` for VERTICAL, a :class:`HorizontalForest` for HORIZONTAL, a
    :class:`TrimmedForest` for TRIM (``pajek_lines`` / ``save_to_pajek`` take them all).
    """
    if pajek_timing not in (VERTICAL, HORIZONTAL, TRIM):
        raise ValueError('pajek_timing must be one of {}, {} or {}, not {!r}'.format(VERTICAL, HORIZONTAL, TRIM, pajek_timing))
    if int(tip_size_threshold) < 0:
        raise ValueError('tip_size_threshold must not be negative, got {}'.format(tip_size_threshold))
    if pajek_timing != TRIM:
        return compress_forest(forest, columns, column2states, timing=pajek_timing, tip_size_threshold=tip_size_threshold,
                               can_merge_diff_sizes=can_merge_diff_sizes, device=device, engine=engine)
    merged = compress_forest(forest, columns, column2states, timing=HORIZONTAL, tip_size_threshold=tip_size_threshold,
                             can_merge_diff_sizes=can_merge_diff_sizes, device=device, engine=engine)
    return trim(merged, tip_size_threshold=tip_size_threshold, can_merge_diff_sizes=can_merge_diff_sizes, device=device,
                engine=engine)


def main(argv=None):
    """The map of a finished run: the named tree and the combined ancestral-state table that the pipeline wrote -> Pajek."""
    import argparse
    import pandas as pd
    from pastml_amd.annotation import preannotate_forest
    from pastml_amd.tree import read_forest
    parser = argparse.ArgumentParser(prog='python -m pastml_amd.visualisation.tree_compressor', description=main.__doc__)
    parser.add_argument('--tree', required=True, help='the named tree of the run (newick, one tree per line)')
    parser.add_argument('--states', required=True, help='its combined ancestral-state table (tab-separated, first column: node)')
    parser.add_argument('--columns', nargs='*', default=None, help='the columns to compress over (default: all of the table)')
    parser.add_argument('--pajek', required=True, help='the file to write')
    parser.add_argument('--pajek_timing', default=VERTICAL, choices=[VERTICAL, HORIZONTAL, TRIM])
    parser.add_argument('--trim', action='store_true', help='the map after trimming (with --pajek_timing left at its default)')
    parser.add_argument('--tip_size_threshold', type=int, default=REASONABLE_NUMBER_OF_TIPS)
    parser.add_argument('--host', action='store_true', help='numpy only, no GPU')
    parser.add_argument('--timeline', default=None, metavar='OUT',
                        help='also write the timeline of the map as a table (pastml_amd.visualisation.timeline)')
    parser.add_argument('--root_date', nargs='+', default=None, metavar='D',
                        help='date of the root(s), for --timeline: one for all trees or one per tree; a number or a calendar date')
    parser.add_argument('--timeline_type', default='SAMPLED', choices=['SAMPLED', 'NODES', 'LTT'])
    args = parser.parse_args(argv)
    if args.timeline:
        from pastml_amd import sharding
        world = sharding.rank_world()[1]
        if world > 1:
            raise NotImplementedError('--timeline is not supported under a multi-process launch ({} ranks): run it in a single '
                                      'process'.format(world))
    roots = read_forest(args.tree)
    df = pd.read_csv(args.states, sep='\t', index_col=0, header=0, dtype=str, keep_default_na=False)
    df.index = df.index.map(str)
    columns = list(df.columns) if not args.columns else list(args.columns)
    missing = [c for c in columns if c not in df.columns]
    if missing:
        raise ValueError('columns {} are not in {}'.format(', '.join(missing), args.states))
    df = df[columns]
    preannotate_forest(roots, df=df)
    column2states = {c: np.array(sorted(set(df[c]) - {''})) for c in columns}
    if args.trim and args.pajek_timing != VERTICAL:
        parser.error('--trim goes with --pajek_timing left at its default')
    if args.trim:
        result = compress_tree(roots, columns, column2states, tip_size_threshold=args.tip_size_threshold, pajek_timing=TRIM,
                               device=False if args.host else None)
    else:
        result = compress_forest(roots, columns, column2states, timing=args.pajek_timing,
                                 tip_size_threshold=args.tip_size_threshold, device=False if args.host else None)
    save_to_pajek(result, columns, args.pajek)
    if args.timeline:
        from pastml_amd.tree import parse_date
        from pastml_amd.visualisation.timeline import timeline, write_timeline
        root_dates = [parse_date(d) for d in args.root_date] if args.root_date else None
        write_timeline(timeline(result, root_dates=root_dates, timeline_type=args.timeline_type, device=False if args.host else None),
                       result, args.timeline)
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
