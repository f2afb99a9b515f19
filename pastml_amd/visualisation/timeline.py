"""
The timeline of the compressed map: what the slider of the reference's compressed visualisation shows at each milestone
(pastml/visualisation/cytoscape_manager.py: the ``get_date`` of the three ``timeline_type``s and the milestone choice in
``visualize`` :751-781, ``update_milestones`` :832-852, the milestone loop of ``_forest2json_compressed`` :219-268 with
``set_cyto_features_compressed`` :104-142) -- for every vertex of the map and every milestone the configurations that already
exist, the tips and internal nodes inside them and the tips below.  Sizes, fonts, colours, coordinates and the HTML are not
produced.

The reference deletes the too recent nodes from an ete3 copy of the full tree and re-filters the vertices' Python lists once per
milestone.  Here it is a closed form over arrays.  From the forest that ``compress_tree`` returned (a ``CompressedForest``
counts as one configuration per vertex), on the host:

    alive  bool[N]   the node is still in the reference's full tree after ``remove_small_tips`` and ``remove_mediators``: not in
                     a removed vertex (nor below one), no internal node left without an alive original tip below it (the
                     clean-up loop of ``remove_small_tips``), no counted internal node of a spliced mediator
    up     int32[N]  the nearest alive ancestor (``remove_mediators`` re-attaches the children to the grandparent), -1 for roots
    config int32[N]  index into ``members`` of the configuration an alive node is inside, -1 for none (a vertex below a
                     configuration that was merged into its sibling belongs to no live vertex, yet its nodes stay in the tree)
    top    int32[C]  the ROOTS node of every configuration;  is_tip bool[N] the original tips

``get_date`` is the date (NODES), the date of ``up`` + 1e-6 below a root (LTT), or the minimum date over the alive original tips
below, ``max_date`` -- the maximum over ALL original tips -- where there is none (SAMPLED).  With milestones m_0 < ... < m_{M-1}:
``bin[n]`` is the first i with ``get_date[n] <= m_i`` (M: none), ``dbin`` the same for the date, ``cbin[x]`` the minimum ``bin``
over the alive nodes whose ``up`` is x.  For configuration c at milestone i, where ``bin[top_c] <= i``:

    tips_inside      alive nodes of c with bin <= i that are an original tip or have cbin > i (the reference counts an internal
                     node whose children are all still hidden as a tip)
    internal_inside  alive internal nodes of c with max(bin, cbin) <= i
    tips_below       original tips under top_c in the ORIGINAL tree with dbin <= i (TIPS_BELOW is fixed when ``compress_tree``
                     starts and is filtered by the plain date)

Under LTT the lists of a vertex (its tips, internal nodes and ROOTS) use ``min(bin, dbin)`` in the place of ``bin``, while
``cbin`` stays the minimum of the children's ``bin``: the reference evaluates ``get_date`` of a node that it has just cut out of
the full tree -- a root by then -- as the node's own date and not as its parent's + 1e-6.  The two differ only where a branch is
shorter than 1e-6 (a zero-length branch: the node is listed at its parent's milestone although it is not in the tree yet).

IS_POLYTOMY nodes are in neither count (``compress_tree`` :94).  A vertex has ``n_roots`` -- its configurations with
``bin[top] <= i`` --, the minimum and maximum over those of each count, and ``first_milestone``, the first i with
``n_roots > 0`` (the reference's MILESTONE feature; M for never).  This equals the reference's loop whenever ``get_date`` does
not decrease from a node to its children (non-negative branch lengths without contradicting given dates); where it does, a
ValueError names the node.  Negative branch lengths are not emulated.

``timeline_host`` is all of this in numpy, with no bound on M; the device path (``Engine.timeline``, pml_timeline) takes at most
64 milestones and is checked against it bit for bit.
"""
import logging

import numpy as np

from pastml_amd.visualisation.tree_compressor import HorizontalForest, TrimmedForest, global_preorder, _engine_for

SAMPLED = 'SAMPLED'
NODES = 'NODES'
LTT = 'LTT'
TIMELINE_TYPES = (SAMPLED, NODES, LTT)
MAX_MILESTONES = 64

# the reference's feature names (tree_compressor.py:19-21, cytoscape_manager.py:59-62)
TIPS_INSIDE = 'in_tips'
INTERNAL_NODES_INSIDE = 'in_ns'
TIPS_BELOW = 'all_tips'
EDGE_NAME = 'edge_name'
MILESTONE = 'mile'

COUNTS = ('n_roots', 'tips_min', 'tips_max', 'internal_min', 'internal_max', 'below_min', 'below_max')


class TimelineArrays(object):
    """The arrays of the module's docstring, derived from a compressed forest: ``flat``, ``alive``, ``up``, ``config``,
    ``is_tip``, ``is_polytomy`` [N]; ``top``, ``below_lo``, ``below_hi`` [C] (the tips below ``top`` are
    ``tip_order[below_lo:below_hi]``); ``tip_order`` [T], the tips in left-to-right leaf order; ``member_offsets`` [L + 1]."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _runs(begin, count):
    """The indices begin[0] .. begin[0] + count[0] - 1, begin[1] .., one run after the other."""
    ends = np.cumsum(count)
    total = int(ends[-1]) if len(ends) else 0
    return np.repeat(begin - (ends - count), count) + np.arange(total)


def timeline_arrays(compressed):
    """:class:`TimelineArrays` of what ``compress_tree`` returned (host, array passes over the depth levels)."""
    from pastml_amd.tree import _polytomy_flags
    if isinstance(compressed, HorizontalForest):
        cf = compressed.compressed
        members = np.asarray(compressed.members, dtype=np.int64)
        member_offsets = np.asarray(compressed.member_offsets, dtype=np.int64)
    else:
        cf = compressed
        members = np.argsort(cf.order).astype(np.int64)   # Pajek order
        member_offsets = np.arange(cf.n_vertices + 1, dtype=np.int64)
    flat = cf.flat
    V, C = cf.n_vertices, len(members)
    parent = flat.parent.astype(np.int64)
    offsets = flat.td_offsets
    levels = [(int(offsets[d]), int(offsets[d + 1])) for d in range(1, len(offsets) - 1)]   # below the roots
    row = np.asarray(cf.vertex_of_node, dtype=np.int64)
    is_tip = np.asarray(flat.is_tip, dtype=bool)
    poly = _polytomy_flags(flat)
    counted = is_tip | ~poly   # what is in TIPS_INSIDE or INTERNAL_NODES_INSIDE of its vertex

    removed_row = np.zeros(V, dtype=bool)
    mediator_row = np.zeros(V, dtype=bool)
    if isinstance(compressed, TrimmedForest):
        before = compressed.horizontal
        entry = np.full(V, -1, dtype=np.int64)
        entry[before.vertex] = np.arange(before.n_vertices)
        gone_entries = entry[np.asarray(compressed.removed, dtype=np.int64)]
        begin = np.asarray(before.member_offsets, dtype=np.int64)[:-1][gone_entries]
        count = np.diff(before.member_offsets)[gone_entries]
        removed_row[np.asarray(before.members, dtype=np.int64)[_runs(begin, count)]] = True
        mediator_row[np.asarray(compressed.mediators, dtype=np.int64)] = True

    # remove_small_tips: the listed nodes of a removed vertex are cut out of the full tree with everything below them ...
    gone = removed_row[row] & counted
    for a, b in levels:
        gone[a:b] |= gone[parent[a:b]]
    # ... and the internal nodes that are left without a tip are cleaned up
    live_tips = (is_tip & ~gone).astype(np.int64)
    for a, b in reversed(levels):
        np.add.at(live_tips, parent[a:b], live_tips[a:b])
    cleaned = ~gone & ~is_tip & (live_tips == 0) & (parent >= 0)
    spliced = mediator_row[row] & ~is_tip & ~poly & ~gone & ~cleaned
    alive = ~(gone | cleaned | spliced)

    up = parent.copy()
    for a, b in levels:
        p = parent[a:b]
        up[a:b] = np.where(alive[p], p, up[p])
    config_of_row = np.full(V, -1, dtype=np.int64)
    config_of_row[members] = np.arange(C)
    config = np.where(alive, config_of_row[row], -1)
    top = np.asarray(cf.top, dtype=np.int64)[members]

    pre = global_preorder(flat)
    tips = flat.tips.astype(np.int64)
    tip_order = tips[np.argsort(pre[tips], kind='stable')]
    tip_pre = pre[tip_order]
    below_lo = np.searchsorted(tip_pre, pre[top])
    below_hi = np.searchsorted(tip_pre, pre[top] + flat.subtree_size[top])
    return TimelineArrays(flat=flat, alive=alive, up=up.astype(np.int32), config=config.astype(np.int32), is_tip=is_tip,
                          is_polytomy=poly, top=top.astype(np.int32), below_lo=below_lo.astype(np.int32),
                          below_hi=below_hi.astype(np.int32), tip_order=tip_order.astype(np.int32),
                          member_offsets=member_offsets.astype(np.int32))


def get_date_host(arrays, date, timeline_type):
    """float64[N]: ``get_date`` of every node (SAMPLED: over the alive tips below it in the original tree, which for an alive
    node are those of its subtree in the ``up`` tree)."""
    flat = arrays.flat
    if timeline_type == NODES:
        return date.copy()
    if timeline_type == LTT:
        return np.where(arrays.up >= 0, date[np.maximum(arrays.up, 0)] + 1e-6, date)
    if timeline_type != SAMPLED:
        raise ValueError('Unknown timeline type: {}. Allowed ones are {}, {} and {}.'.format(timeline_type, NODES, SAMPLED, LTT))
    earliest = np.where(arrays.alive & arrays.is_tip, date, np.inf)
    offsets = flat.td_offsets
    for d in range(len(offsets) - 2, 0, -1):
        a, b = int(offsets[d]), int(offsets[d + 1])
        np.minimum.at(earliest, flat.parent[a:b], earliest[a:b])
    return np.where(np.isinf(earliest), date[arrays.is_tip].max(), earliest)


def choose_milestones(arrays, date, timeline_type):
    """The reference's milestones: nine order statistics of the dates of all nodes (NODES, LTT) or all tips (SAMPLED) of the
    untrimmed forest as a set (``visualize`` :766-773), then ``update_milestones`` over what the trimming left."""
    everything = timeline_type in (NODES, LTT)
    pool = date if everything else date[arrays.is_tip]
    n = len(pool)
    at = sorted({0, n // 8, n // 4, 3 * n // 8, n // 2, 5 * n // 8, 3 * n // 4, 7 * n // 8, n - 1})
    milestones = sorted(set(np.partition(pool, at)[at].tolist()))
    left = date[arrays.alive] if everything else date[arrays.alive & arrays.is_tip]
    first, last = float(left.min()), float(left.max())
    milestones = [m for m in milestones if first <= m <= last] or [first]   # (the reference fails on an empty list)
    if milestones[0] > first:
        milestones.insert(0, first)
    if milestones[-1] < last:
        milestones.append(last)
    return np.array(milestones, dtype=np.float64)


def milestone_labels(milestones, dates_are_dates):
    from pastml_amd.tree import numeric2datetime
    if dates_are_dates:
        try:
            return [numeric2datetime(m).strftime('%d %b %Y') for m in milestones]
        except Exception:   # (as the reference: whatever fails, the numbers are shown)
            pass
    return ['{:g}'.format(m) for m in milestones]


def _checked_milestones(milestones):
    milestones = np.asarray(milestones, dtype=np.float64).reshape(-1)
    if len(milestones) < 1:
        raise ValueError('at least one milestone is needed')
    if np.isnan(milestones).any() or (np.diff(milestones) <= 0).any():
        raise ValueError('the milestones must be sorted in strictly ascending order')
    return milestones


def check_monotone(arrays, get_date):
    """ValueError where ``get_date`` decreases from an alive node to an alive child: the closed form is not the reference's loop.
    (Under LTT the caller passes the dates: ``get_date`` is the parent's date there, and the lists look at a node's own.)"""
    child = np.flatnonzero(arrays.alive & (arrays.up >= 0))
    bad = child[get_date[child] < get_date[arrays.up[child]]]
    if len(bad):
        n = int(bad[0])
        nodes = arrays.flat.nodes
        name = nodes[n].name if nodes is not None else 'n{}'.format(n)
        raise ValueError('get_date decreases from node {!r} ({}) to its child {!r} ({}): negative branch lengths or given dates that '
                         'contradict the tree are not supported'.format(
                             nodes[int(arrays.up[n])].name if nodes is not None else 'n{}'.format(int(arrays.up[n])),
                             get_date[arrays.up[n]], name, get_date[n]))


def counts_host(arrays, date, get_date, milestones, timeline_type=SAMPLED):
    """dict of the seven int32[L, M] arrays of ``COUNTS`` and ``first_milestone`` int32[L] (numpy, no bound on M)."""
    m = np.asarray(milestones, dtype=np.float64)
    M = len(m)
    C, L = len(arrays.top), len(arrays.member_offsets) - 1
    alive, up, config = arrays.alive, arrays.up.astype(np.int64), arrays.config.astype(np.int64)
    bins = np.searchsorted(m, get_date, side='left')
    cbin = np.full(len(bins), M, dtype=np.int64)
    child = np.flatnonzero(alive & (up >= 0))
    np.minimum.at(cbin, up[child], bins[child])
    if timeline_type == LTT:   # (the lists: a node cut out of the tree answers with its own date, see the module docstring)
        bins = np.where(up >= 0, np.minimum(bins, np.searchsorted(m, date, side='left')), bins)

    inside = alive & (config >= 0) & ~arrays.is_polytomy
    tips = np.zeros((C, M + 1), dtype=np.int64)
    internal = np.zeros((C, M + 1), dtype=np.int64)
    x = np.flatnonzero(inside & arrays.is_tip)
    np.add.at(tips, (config[x], bins[x]), 1)
    x = np.flatnonzero(inside & ~arrays.is_tip)
    hidden = x[cbin[x] > bins[x]]   # a tip from its own bin until the first child shows
    np.add.at(tips, (config[hidden], bins[hidden]), 1)
    np.add.at(tips, (config[hidden], cbin[hidden]), -1)
    np.add.at(internal, (config[x], np.maximum(bins[x], cbin[x])), 1)
    tips = np.cumsum(tips, axis=1)[:, :M]
    internal = np.cumsum(internal, axis=1)[:, :M]

    tbin = np.searchsorted(m, date[arrays.tip_order], side='left')
    below = np.zeros((C, M), dtype=np.int64)
    for j in np.unique(tbin[tbin < M]):
        before = np.concatenate(([0], np.cumsum(tbin == j)))
        below[:, j] = before[arrays.below_hi] - before[arrays.below_lo]
    below = np.cumsum(below, axis=1)

    starts = arrays.member_offsets[:-1].astype(np.int64)
    if (np.diff(arrays.member_offsets) < 1).any():
        raise ValueError('a vertex without a configuration')
    shown = bins[arrays.top][:, None] <= np.arange(M)[None, :]
    out = {'n_roots': np.add.reduceat(shown.astype(np.int64), starts, axis=0)}
    some = out['n_roots'] > 0
    big = np.iinfo(np.int64).max
    for name, values in (('tips', tips), ('internal', internal), ('below', below)):
        out[name + '_min'] = np.where(some, np.minimum.reduceat(np.where(shown, values, big), starts, axis=0), 0)
        out[name + '_max'] = np.maximum.reduceat(np.where(shown, values, 0), starts, axis=0)
    out = {name: out[name].astype(np.int32).reshape(L, M) for name in COUNTS}
    out['first_milestone'] = np.where(some.any(axis=1), np.argmax(some, axis=1), M).astype(np.int32)
    return out


def timeline_host(arrays, root_dates=None, given_dates=None, timeline_type=SAMPLED, milestones=None):
    """
    The timeline in numpy: dict of ``milestones``, ``date``, ``get_date`` float64 and the arrays of ``counts_host``.  No bound on
    the number of milestones.  ``arrays``: :func:`timeline_arrays` of the compressed forest.
    """
    from pastml_amd.tree import annotate_dates
    date = annotate_dates(arrays.flat, root_dates, given_dates)
    get_date = get_date_host(arrays, date, timeline_type)
    check_monotone(arrays, date if timeline_type == LTT else get_date)
    milestones = choose_milestones(arrays, date, timeline_type) if milestones is None else _checked_milestones(milestones)
    out = counts_host(arrays, date, get_date, milestones, timeline_type)
    out.update(milestones=milestones, date=date, get_date=get_date)
    return out


def timeline_device(arrays, engine, root_dates=None, given_dates=None, timeline_type=SAMPLED, milestones=None):
    """The same from ``engine.timeline`` (pml_timeline): without milestones one call for the dates, the reference's choice on the
    host from the downloaded array, and one call for everything."""
    from pastml_amd.tree import root_date_array
    flat = arrays.flat
    if timeline_type not in TIMELINE_TYPES:
        raise ValueError('Unknown timeline type: {}. Allowed ones are {}, {} and {}.'.format(timeline_type, NODES, SAMPLED, LTT))
    given = np.full(flat.n_nodes, np.nan) if given_dates is None else np.asarray(given_dates, dtype=np.float64)
    nodes = (flat.td_offsets, flat.parent, flat.dist, given, root_date_array(flat, root_dates))
    if milestones is None:
        milestones = choose_milestones(arrays, engine.timeline(*nodes), timeline_type)
    else:
        milestones = _checked_milestones(milestones)
    out = engine.timeline(*nodes, alive=arrays.alive, up=arrays.up, config=arrays.config, is_tip=arrays.is_tip,
                          is_polytomy=arrays.is_polytomy, top=arrays.top, below_lo=arrays.below_lo, below_hi=arrays.below_hi,
                          tip_order=arrays.tip_order, member_offsets=arrays.member_offsets, timeline_type=timeline_type,
                          milestones=milestones)
    check_monotone(arrays, out['date'] if timeline_type == LTT else out['get_date'])
    out['milestones'] = milestones
    return out


def _min_max_str(lo, hi):
    """``get_min_max_str`` of the reference: ' a-b', or ' a' where both are one."""
    return ' {}'.format('{}-{}'.format(lo, hi) if lo != hi else lo)


class Timeline(object):
    """
    The timeline of a compressed forest, vertices in Pajek order (the entries of a ``HorizontalForest`` / ``TrimmedForest``, the
    ranks of a ``CompressedForest``):

        milestones, labels                 float64[M], their texts
        timeline_type
        date, get_date                     float64[N]
        n_roots                            int32[L, M]  configurations of the vertex that exist at the milestone
        tips_min, tips_max                 int32[L, M]  tips inside, minimum and maximum over those configurations
        internal_min, internal_max         int32[L, M]  internal nodes inside
        below_min, below_max               int32[L, M]  tips below
        first_milestone                    int32[L]     the first milestone with n_roots > 0 (M: never)
        alive, up, config, top             the arrays they were counted from
    """

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @property
    def n_vertices(self):
        return len(self.first_milestone)

    def features(self, v=None):
        """
        The reference's features of vertex v (all vertices: a list) as ``_forest2json_compressed`` leaves them: ``mile`` and, for
        every milestone i at which the vertex exists, ``node_in_tips_i``, ``node_in_ns_i``, ``node_all_tips_i`` and
        ``edge_name_i``.  Empty with a single milestone: the reference writes no timeline features then.
        """
        if v is None:
            return [self.features(i) for i in range(self.n_vertices)]
        M = len(self.milestones)
        out = {}
        if M < 2:
            return out
        first = int(self.first_milestone[v])
        if first < M:
            out[MILESTONE] = first
        for i in range(first, M):
            suffix = '_{}'.format(i)
            n = int(self.n_roots[v, i])
            out['node_{}{}'.format(TIPS_INSIDE, suffix)] = _min_max_str(int(self.tips_min[v, i]), int(self.tips_max[v, i]))
            out['node_{}{}'.format(INTERNAL_NODES_INSIDE, suffix)] = _min_max_str(int(self.internal_min[v, i]),
                                                                                 int(self.internal_max[v, i]))
            out['node_{}{}'.format(TIPS_BELOW, suffix)] = _min_max_str(int(self.below_min[v, i]), int(self.below_max[v, i]))
            out['{}{}'.format(EDGE_NAME, suffix)] = str(n) if n != 1 else ''
        return out


def timeline(compressed, root_dates=None, given_dates=None, timeline_type=SAMPLED, milestones=None, dates_are_dates=None,
             device=None, engine=None):
    """
    The :class:`Timeline` of what ``compress_tree`` returned.

    :param root_dates: the date of the roots without a given date: one for all trees or one per tree (default 0)
    :param given_dates: float64[N] over the nodes of the flat forest, NaN where no date is given
    :param timeline_type: SAMPLED, NODES or LTT
    :param milestones: sorted dates, at most 64; None for the reference's choice
    :param dates_are_dates: label the milestones as calendar dates (default: when root or given dates were passed)
    :param device: None -- the GPU when there is one, else numpy; False -- numpy; True or an index -- the GPU, or an error
    :param engine: a hip.Engine to use for its device and stream
    """
    if timeline_type not in TIMELINE_TYPES:
        raise ValueError('Unknown timeline type: {}. Allowed ones are {}, {} and {}.'.format(timeline_type, NODES, SAMPLED, LTT))
    if milestones is not None:
        milestones = _checked_milestones(milestones)
        if len(milestones) > MAX_MILESTONES:
            raise ValueError('{} milestones: at most {} are supported'.format(len(milestones), MAX_MILESTONES))
    arrays = timeline_arrays(compressed)
    eng, release = _engine_for(arrays.flat, 1, device, engine, 'Timeline')
    try:
        if eng is None:
            out = timeline_host(arrays, root_dates, given_dates, timeline_type, milestones)
        else:
            out = timeline_device(arrays, eng, root_dates, given_dates, timeline_type, milestones)
    finally:
        release()
    if dates_are_dates is None:
        dates_are_dates = root_dates is not None or given_dates is not None
    logging.getLogger('pastml').debug('Timeline of {} vertices at {} milestones ({}).'.format(
        len(out['first_milestone']), len(out['milestones']), timeline_type))
    return Timeline(labels=milestone_labels(out['milestones'], dates_are_dates), timeline_type=timeline_type, alive=arrays.alive,
                    up=arrays.up, config=arrays.config, top=arrays.top, **out)


def write_timeline(timeline, compressed, path):
    """
    Writes the timeline as a tab-separated table, one row per (milestone, live vertex with at least one configuration at it):
    milestone label, Pajek id, vertex name, roots, tips inside, internal nodes inside, tips below -- the last three as the
    reference's min-max texts ('3' or '1-4').  The reference has no such file: it keeps these numbers inside its HTML.
    """
    if isinstance(compressed, HorizontalForest):
        names = compressed.compressed.name[compressed.vertex]
    else:
        names = compressed.name[np.argsort(compressed.order)]
    with open(path, 'w+') as f:
        f.write('milestone\tid\tvertex\troots\ttips_inside\tinternal_nodes_inside\ttips_below\n')
        for i, label in enumerate(timeline.labels):
            for v in np.flatnonzero(timeline.n_roots[:, i] > 0).tolist():
                f.write('{}\t{}\t{}\t{}\t{}\t{}\t{}\n'.format(
                    label, v + 1, names[v], timeline.n_roots[v, i],
                    _min_max_str(timeline.tips_min[v, i], timeline.tips_max[v, i])[1:],
                    _min_max_str(timeline.internal_min[v, i], timeline.internal_max[v, i])[1:],
                    _min_max_str(timeline.below_min[v, i], timeline.below_max[v, i])[1:]))
