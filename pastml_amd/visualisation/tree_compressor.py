"""
The compressed tree of a reconstruction, vertical step (pastml/visualisation/tree_compressor.py: ``collapse_vertically``
:251-298 on the lists ``compress_tree`` :87-96 starts from), and its Pajek network (``_tree2pajek_vertices_arcs`` :34-51,
``save_to_pajek`` :54-80) -- what the reference writes at its default ``pajek_timing='VERTICAL'``.

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

Horizontal merging, trimming, focus / mixed mode (the rest of ``compress_tree``) are not implemented.
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
    (vertex lines, arc lines) of the reference's ``_tree2pajek_vertices_arcs`` at vertical timing, the trees of the forest
    in turn with ids that continue.  ``<tips>`` joins the tips inside by ';': at this timing the reference's TIPS_INSIDE is
    still a flat list, so its outer ';'.join runs over single tips.
    """
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
    <source_id> <target_id> 1
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
