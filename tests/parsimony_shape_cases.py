"""
TEST INFRASTRUCTURE: the forests, state counts and annotations on which tests/test_gpu_parsimony_shapes.py holds the parsimony
passes of the device (pml_kernels_parsimony.h, pml_launch_parsimony.hip) to the reference (tests/golden/parsimony_shapes.npz,
written by tests/golden/make_golden_parsimony_shapes.py), and a restatement of the kernels' bit-sliced counters with which
tests/test_parsimony_shape_cases_host.py shows that those comparisons can fail.  Host arithmetic only: the host file holds every
case listed here to what it is for, so that the GPU file filters nothing.

Forests (an engine each: the launcher picks the number of counter planes P per forest, from its largest arity):

    shapes, crowd, grafted    degenerate_forest_cases.forest(name): unary nodes, lone tips, roots over one tip, stars up to 17 tips;
                              501 tiny trees (levels wider than PARS_THIN = 512 units); unary nodes spliced into polytomies
    arity_a                   a in ARITIES: a root star of a tips; root -> [tip, inner node with a tips] (the inner node's "up" set is a
                              set of its own, not all states); stars of 2 and of 3 tips (those of at most a: the largest arity is a
                              exactly); a lone tip; root -> unary -> tip
    arity_65534, arity_65535  a root star of a tips, stars of 2 and 3, a lone tip, root -> unary -> tip.  Beyond the reference's reach
                              (its downpass is quadratic in the arity): held to the host path and to CLOSED FORMS

P (planes_for): 2 up to 2 children, 4 up to 14, 8 up to 254, 16 up to 65534, 32 beyond -- a count reaches arity + 1 (the parent's "up"
set and every child) and P planes hold 2^P - 1.

State counts: K_ALL gives W = 1 .. 8 words, every group width WG = 1, 2, 4, 8 and dead lanes at W = 3, 5, 6, 7; the last word is
once full and once a single bit.

Columns of a case (one pml_parsimony call), s0 = 0 and s1 = k - 1:

    0  unanimous: every tip {s1}.  Every node {s1}, 0 steps; the count of s1 at a node of arity a in DOWN is a + 1
    1  all but one: column 0 with the first child of every node of the largest arity {s0}
    2  tie across words (k >= 2): the children of every internal node alternate {s0}, {s1}; an odd last child has no data.  A star
       of even arity: root {s0, s1}, a / 2 steps
    3  palette: a tip takes one of {0, k - 1, 64 w, 64 w + 63}, 15 % take three of them and 10 % none; 10 % of the internal nodes --
       and one unary node, one internal root -- are annotated with two
    4  random_given of tests/test_gpu_parsimony.py
    5  every tip {s1}, every internal node {s0}: no intersection anywhere, the "own set wins" branch of pars_restrict
"""
import functools

import numpy as np

import degenerate_forest_cases as degenerate
from pastml_amd import parsimony as P
from pastml_amd.batch import masks_from_words
from pastml_amd.hip import pack_masks
from pastml_amd.tree import FlatForest
from test_gpu_parsimony import random_given

ARITIES = (2, 3, 14, 15, 254, 255, 256)
BIG_ARITIES = (65534, 65535)
FIXTURE_FORESTS = degenerate.FORESTS + tuple('arity_{}'.format(a) for a in ARITIES)
BIG_FORESTS = tuple('arity_{}'.format(a) for a in BIG_ARITIES)
FORESTS = FIXTURE_FORESTS + BIG_FORESTS
PLANES = dict(zip(FORESTS, (8, 4, 4, 2, 4, 4, 8, 8, 16, 16, 16, 32)))   # (shapes: 17 children; crowd: 3; grafted: 5)
K_ALL = [1, 2, 63, 64, 65, 128, 129, 192, 193, 320, 321, 448, 449, 512]
K_FEW = [2, 193, 449]
BIG_K_DEVICE = (2, 193)   # the state counts at which the GPU file runs the two big forests
N_COLUMNS = 6
METHODS = (P.ACCTRAN, P.DOWNPASS, P.DELTRAN)   # the order of pml_parsimony's slots


def states_of(name):
    if name in ('shapes', 'grafted'):
        return K_ALL
    return K_FEW + [321] if name == 'arity_255' else K_FEW


CASES = [(name, k) for name in FORESTS for k in states_of(name)]
FIXTURE_CASES = [(name, k) for name, k in CASES if name in FIXTURE_FORESTS]
IDS = ['{}-k{}'.format(*c) for c in FIXTURE_CASES]


def planes_for(arity):
    """pml_launch_parsimony.hip, launch_parsimony: the first of 2, 4, 8, 16, 32 planes whose 2^P exceeds arity + 1 (32 at most)."""
    planes = 2
    while planes < 32 and (1 << planes) <= arity + 1:
        planes <<= 1
    return planes


def columns_of(k):
    return [c for c in range(N_COLUMNS) if c != 2 or k >= 2]


def tag(name, k):
    return '{}_k{}_'.format(name, k)


def fixture(z, name, k):
    """(sets uint64 [3, columns, N, W], steps [3, columns]) of the reference, the methods in the order of METHODS; z: parsimony_shapes.npz,
    which keeps the three sets of a node side by side."""
    return np.ascontiguousarray(np.moveaxis(z[tag(name, k) + 'selected'], 2, 0)), z[tag(name, k) + 'steps']


# ---------------------------------------------------------------------------------------------------------------------
# the forests
# ---------------------------------------------------------------------------------------------------------------------
TIP = ()


def star_of(n):
    return (TIP,) * n


def flatten(trees):
    """Nested tuples (a node: the tuple of its children) -> FlatForest, ids breadth-first over the whole forest."""
    nodes = list(trees)
    parent = [-1] * len(nodes)
    first_child, n_children = [], []
    i = 0
    while i < len(nodes):
        first_child.append(len(nodes))
        n_children.append(len(nodes[i]))
        parent.extend([i] * len(nodes[i]))
        nodes.extend(nodes[i])
        i += 1
    dist = np.where(np.array(parent) < 0, 0.0, 0.1)
    return FlatForest(parent, n_children, first_child, dist, np.arange(len(trees)))


def arity_trees(a):
    trees = [star_of(a)]
    if a not in BIG_ARITIES:
        trees.append((TIP, star_of(a)))
    trees += [star_of(s) for s in (2, 3) if s <= a]
    return trees + [TIP, ((TIP,),)]


@functools.lru_cache(maxsize=None)
def forest(name):
    if name in degenerate.FORESTS:
        return degenerate.forest(name)
    return flatten(arity_trees(int(name[len('arity_'):])))


def largest_nodes(flat):
    return np.flatnonzero(flat.n_children == flat.n_children.max())


# ---------------------------------------------------------------------------------------------------------------------
# the annotations
# ---------------------------------------------------------------------------------------------------------------------
def palette(k):
    W = (k + 63) // 64
    return np.unique([s for s in [0, k - 1] + [64 * w for w in range(W)] + [64 * w + 63 for w in range(W)] if s < k])


def _set_bits(words, nodes, states):
    nodes, states = np.broadcast_arrays(np.asarray(nodes, dtype=np.int64), np.asarray(states, dtype=np.int64))
    np.bitwise_or.at(words, (nodes, states // 64), np.uint64(1) << (states % 64).astype(np.uint64))


def _palette_column(flat, k, rng):
    """(words [N, W], restricted unary node or -1, restricted internal root or -1)"""
    nc, W = flat.n_children, (k + 63) // 64
    pal = palette(k)
    words = np.zeros((flat.n_nodes, W), dtype=np.uint64)
    u = rng.random(flat.n_nodes)
    for i in np.flatnonzero(nc == 0):
        if u[i] >= 0.1:
            _set_bits(words, i, rng.choice(pal, size=min(3, len(pal)), replace=False) if u[i] < 0.25 else rng.choice(pal))
    held = set(np.flatnonzero((nc > 0) & (u < 0.1)).tolist())
    unary = np.flatnonzero(nc == 1)
    inner_roots = flat.roots[nc[flat.roots] > 0]
    held_unary = int(unary[int(rng.integers(len(unary)))]) if len(unary) else -1
    held_root = int(inner_roots[int(rng.integers(len(inner_roots)))]) if len(inner_roots) else -1
    for i in sorted(held | {held_unary, held_root} - {-1}):
        _set_bits(words, i, rng.choice(pal, size=min(2, len(pal)), replace=False))
    return words, held_unary, held_root


@functools.lru_cache(maxsize=None)
def build(name, k):
    """dict(name, k, flat, cols (the columns present), given uint64 [len(cols), N, W], restricted_unary, restricted_root (column 3))."""
    assert (name, k) in CASES
    flat = forest(name)
    N, W, nc, fc = flat.n_nodes, (k + 63) // 64, flat.n_children, flat.first_child
    s0, s1 = 0, k - 1
    tips, inner = np.flatnonzero(nc == 0), np.flatnonzero(nc > 0)
    given = np.zeros((N_COLUMNS, N, W), dtype=np.uint64)
    _set_bits(given[0], tips, s1)
    _set_bits(given[1], tips, s1)
    first = fc[largest_nodes(flat)]
    given[1, first] = 0
    _set_bits(given[1], first, s0)
    for p in inner:   # (children are consecutive ids)
        kids = np.arange(fc[p], fc[p] + nc[p] - nc[p] % 2)
        _set_bits(given[2], kids, np.where((kids - fc[p]) % 2 == 0, s0, s1))
    rng = np.random.default_rng(7100 + 10 * k + FORESTS.index(name))
    given[3], held_unary, held_root = _palette_column(flat, k, rng)
    given[4] = random_given(flat, k, 1, seed=7200 + 10 * k + FORESTS.index(name))[0]
    _set_bits(given[5], tips, s1)
    _set_bits(given[5], inner, s0)
    cols = columns_of(k)
    given = np.ascontiguousarray(given[cols])
    given.setflags(write=False)
    return dict(name=name, k=k, flat=flat, cols=cols, given=given, restricted_unary=held_unary, restricted_root=held_root)


# ---------------------------------------------------------------------------------------------------------------------
# the host path, and what it shows about an input
# ---------------------------------------------------------------------------------------------------------------------
def host_passes(flat, given, k):
    """(sets int8 [3, N, k], steps [3]) of one column by pastml_amd.parsimony's host path, in the order of METHODS."""
    g = masks_from_words(given, k).astype(np.int32)
    initial = np.where(g.any(axis=1, keepdims=True), g, 1).astype(np.int32)
    bu = P.uppass(flat, initial)
    down = P.downpass(flat, bu, initial)
    sets = [P.acctran(flat, bu), down, P.deltran(flat, down)]
    return np.stack(sets).astype(np.int8), np.array([P.num_parsimonious_steps(flat, s) for s in sets])


def sets_as_words(sets, k):
    return pack_masks(sets, k)


def down_counts(flat, given, k, node):
    """The counts from which DOWN picks `node`'s set: its "up" set (all states at a root) plus its children's bottom-up sets, [k].
    Plain sums over the path from the root; what parsimony.downpass computes level by level."""
    g = masks_from_words(given, k).astype(np.int64)
    bu = P.uppass(flat, np.where(g.any(axis=1, keepdims=True), g, 1).astype(np.int32)).astype(np.int64)
    nc, fc = flat.n_children, flat.first_child
    path = [int(node)]
    while flat.parent[path[-1]] >= 0:
        path.append(int(flat.parent[path[-1]]))
    up = np.ones(k, dtype=np.int64)
    for p, child in zip(path[:0:-1], path[-2::-1]):
        counts = up + bu[fc[p]:fc[p] + nc[p]].sum(axis=0) - bu[child]
        up = (counts == counts.max()).astype(np.int64)
    return up + bu[fc[node]:fc[node] + nc[node]].sum(axis=0)


def closed_forms(name, k):
    """Of a big forest (a root star of a tips, stars of 2 and 3, a lone tip, root -> unary -> tip), k >= 2: the steps of columns 0, 1,
    2 and 5 (the same for the three methods) and the big root's set in columns 0, 1 and 2 as a list of states."""
    a = int(name[len('arity_'):])
    flat = forest(name)
    assert name in BIG_FORESTS and k >= 2 and flat.n_children[0] == a
    # column 2: a // 2 changes under the big root (its last child has no data when a is odd), one each in the stars of 2 and 3,
    # none under the unary node (its tip and itself are both {s0})
    steps = {0: 0, 1: 1, 2: a // 2 + 2, 5: flat.n_tips - 1}   # (column 5: every tip below an internal node differs from it)
    root = {0: [k - 1], 1: [k - 1], 2: [0, k - 1]}
    return steps, root


def assert_closed_forms(name, k, results):
    """results: {column: (sets 0/1 [3, N, k], steps [3])} of columns 0, 1, 2 and 5 of a big forest."""
    flat = forest(name)
    want_steps, want_root = closed_forms(name, k)
    for col, steps in want_steps.items():
        assert list(results[col][1]) == [steps] * 3, col
    for col, states in want_root.items():
        assert all(np.flatnonzero(results[col][0][j, 0]).tolist() == states for j in range(3)), col
    only_s1 = np.zeros(k, dtype=np.int8)
    only_s1[k - 1] = 1
    assert np.all(results[0][0] == only_s1)                    # column 0: every node {s1}
    others = np.ones(flat.n_nodes, dtype=bool)
    others[flat.first_child[0]] = False                        # column 1: and the big root's first child {s0}
    assert np.all(results[1][0][:, others] == only_s1) and np.all(results[1][0][:, ~others].sum(axis=2) == 1)
    assert np.all(results[1][0][:, ~others, 0] == 1)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' counters, restated: P planes, groups of WG words
# ---------------------------------------------------------------------------------------------------------------------
def _or_of_group(nonzero, W):
    return nonzero.any(axis=1)


def _or_without_last_live_word(nonzero, W):
    """MUTANT: the group OR misses the last live word."""
    return nonzero[:, :max(W - 1, 1)].any(axis=1)


class Planes(object):
    """PmlPlanes<P> for all columns of a case at once: plane j holds bit j of every state's count, [P, C, WG] words."""

    def __init__(self, n_planes, shape):
        self.p = np.zeros((n_planes,) + shape, dtype=np.uint64)

    def copy(self):
        other = Planes(0, self.p.shape[1:])
        other.p = self.p.copy()
        return other

    def add(self, x):
        for plane in self.p:
            carry = plane & x
            plane ^= x
            x = carry

    def sub(self, x):
        for plane in self.p:
            borrow = ~plane & x
            plane ^= x
            x = borrow


def most_common(planes, cand, W, group_or):
    """pars_most_common: (the states of cand [C, WG] with the largest count, that count [C])."""
    maxv = np.zeros(cand.shape[0], dtype=np.int64)
    for j in range(len(planes.p) - 1, -1, -1):
        t = cand & planes.p[j]
        hit = group_or(t != 0, W)
        cand = np.where(hit[:, None], t, cand)
        maxv |= hit.astype(np.int64) << j
    return cand, maxv


def _restrict(own, wanted, W, group_or):
    both = own & wanted
    return np.where(group_or(both != 0, W)[:, None], both, own)


def sliced_passes(flat, given, k, n_planes, group_or=_or_of_group):
    """
    The passes as pars_unit runs them, on counters of n_planes planes and groups of WG = 1, 2, 4 or 8 words of which W are live.
    given: uint64 [C, N, W].  Returns (sets uint64 [3, C, N, W], steps [3, C], the winning count of every internal node in DOWN [C, N]).
    """
    C, N, W = given.shape
    WG = 1 << (W - 1).bit_length()
    nc, fc, parent = flat.n_children, flat.first_child, flat.parent
    every = np.zeros(WG, dtype=np.uint64)
    every[:W] = ~np.uint64(0)
    if k % 64:
        every[W - 1] = (np.uint64(1) << np.uint64(k % 64)) - np.uint64(1)
    every = np.broadcast_to(every, (C, WG))
    init = np.zeros((C, N, WG), dtype=np.uint64)
    init[:, :, :W] = given
    init = np.where(init.any(axis=2, keepdims=True), init, every[:, None, :])

    bu = init.copy()
    for n in flat.bu_order:
        cnt = Planes(n_planes, (C, WG))
        for c in range(fc[n], fc[n] + nc[n]):
            cnt.add(bu[:, c])
        bu[:, n] = _restrict(init[:, n], most_common(cnt, every, W, group_or)[0], W, group_or)

    def restricted(src, dst):
        for n in range(N):   # (parents have smaller ids)
            own = src[:, n].copy()
            dst[:, n] = own if parent[n] < 0 else _restrict(own, dst[:, parent[n]], W, group_or)
        return dst

    down, up = init.copy(), np.zeros_like(init)
    down_max = np.zeros((C, N), dtype=np.int64)
    for n in np.flatnonzero(nc > 0):
        cnt = Planes(n_planes, (C, WG))
        cnt.add(every if parent[n] < 0 else up[:, n])
        for c in range(fc[n], fc[n] + nc[n]):
            cnt.add(bu[:, c])
        mc, down_max[:, n] = most_common(cnt, every, W, group_or)
        down[:, n] = _restrict(init[:, n], mc, W, group_or)
        for c in range(fc[n], fc[n] + nc[n]):
            t = cnt.copy()
            t.sub(bu[:, c])
            upc = most_common(t, every, W, group_or)[0]
            if nc[c] > 0:
                up[:, c] = upc
            else:
                down[:, c] = _restrict(init[:, c], upc, W, group_or)

    def steps_of(sets):
        z, m = sets.copy(), np.zeros((C, N), dtype=np.int64)
        for n in flat.bu_order:
            cnt = Planes(n_planes, (C, WG))
            for c in range(fc[n], fc[n] + nc[n]):
                cnt.add(z[:, c])
            z[:, n], maxv = most_common(cnt, sets[:, n], W, group_or)
            m[:, n] = m[:, fc[n]:fc[n] + nc[n]].sum(axis=1) + nc[n] - maxv
        return m[:, flat.roots].sum(axis=1)

    sets = [restricted(bu, np.zeros_like(bu)), down, restricted(down, down.copy())]
    return np.stack(sets)[..., :W], np.stack([steps_of(s) for s in sets]), down_max


MUTANT_HALF_PLANES = 'half the planes'
MUTANT_GROUP_OR = 'group OR without the last live word'


def mutant_passes(mutant, flat, given, k):
    n_planes = planes_for(int(flat.n_children.max()))
    if mutant == MUTANT_HALF_PLANES:
        return sliced_passes(flat, given, k, n_planes // 2)
    assert mutant == MUTANT_GROUP_OR
    return sliced_passes(flat, given, k, n_planes, _or_without_last_live_word)
