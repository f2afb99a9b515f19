"""
TEST INFRASTRUCTURE: the inputs on which the sum sweeps and the joint sweep of the matrix models (eigen models, HKY) are held to
exact arithmetic (tests/matrix_exact_ref.py), shared by tests/test_matrix_exact_ref.py (the oracle, CPU) and
tests/test_gpu_eigen_shapes.py, tests/test_gpu_joint_shapes.py (the device).  Host arithmetic only.

For a state count k:

    forest S   some 60 nodes, up to four children per node, two trees, no zero-length branch: the tip launch and the
               several-levels-per-launch ("narrow") kernel.
    forest L   by hand: a root, 2 children, 4 children each, 17 children each, every one of those 136 a cherry of 2 tips
               (419 nodes).  Bottom-up the 136 cherries are one level above the narrow limit of the two-GEMM sweeps
               (2 x 4 waves x 16 = 128 nodes), the levels above (8, 2, 1) its narrow end; the 8 nodes of 17 children run the odd
               tail of the pair loop over children.  Top-down the depths hold 2, 8, 136 and 272 nodes: the first two are the
               narrow launch (a single narrow depth gets no launch of its own kind -- pml_schedule.cpp, narrow_levels -- which is
               why the 8 hang under 2 nodes and not under the root), the cherries and the tips a level launch each.
    forest J   (joint sweep) by hand: a root, 2 children, n cherries under them: one level launch of the joint kernels over n nodes,
               n chosen per k for three passes per wave (j_cherries), and the narrow launch above.
    forest T   (joint sweep beyond 64 states) ((a,b),(c,d),e).
    column 0   every tip observed (the gathered first product of the tip launch), tau = 0, tf = 1.
    column 1   random_masks: missing and ambiguous tips, restricted internal nodes; tau > 0, tf < 1.  Its own model and rates.

Deep forests (rescaling): a caterpillar with one observed tip per level whose depth is read from the exact bottom-up sweep, and a
forest of small trees whose polytomies of observed tips leave the rescaling band inside one node's loop over its children.
"""
import functools

import numpy as np

import matrix_exact_ref as exact
from oracle import pastml_oracle as orc
from pastml_amd import synthetic
from pastml_amd.tree import FlatForest, TreeNode
from test_gpu_parity import LNL_RTOL, LOG10_ATOL, POST_RTOL, random_masks, random_spec

STATES_TWO_MATRICES = list(range(2, 65))                  # A and A^-1 as operands: every lane shape below 65 states
STATES_ONE_MATRIX = [65, 80, 81, 96, 97, 112, 113, 128]   # the one-matrix form at its shape boundaries
LOG10_ATOL_ONE_MATRIX = 1e-9                              # (test_eigen_sum_sweeps_of_65_to_128_states)
JOINT_STATES = [11, 23, 43, 51, 58]
# the state counts the suite never ran top-down (KS 3, 6, 11, 13, 15), bottom-up KS 14, the k of the level kernels it did run,
# and the boundaries of the register / LDS forms
CPU_STATES = sorted(set([2, 4, 5, 16, 17, 20, 32, 33, 53, 61, 64] + list(range(9, 13)) + list(range(21, 25)) + list(range(41, 45))
                        + list(range(49, 61))))
# ... of which the oracle is run on forest L as well (the other L cases differ from these in k only, and cost seconds each)
CPU_STATES_L = [2, 5, 9, 12, 21, 24, 41, 44, 52, 53, 57, 60, 64]
MIN_MESSAGE_RATIO = 1e-9
S_TIPS = 40
L_SHAPE = (2, 4, 17)    # children of the root, of those, of those; then cherries


def log10_atol(k):
    return LOG10_ATOL if k <= 64 else LOG10_ATOL_ONE_MATRIX


@functools.lru_cache(maxsize=None)
def forest_s(k):
    return FlatForest.random(S_TIPS, seed=900 + k, max_arity=4, zero_frac=0.0, lo=0.01, n_trees=2)


@functools.lru_cache(maxsize=None)
def forest_l():
    rng = np.random.default_rng(417)
    root = TreeNode(name='r', dist=0.0)
    level = [root]
    for fan in L_SHAPE + (2,):
        level = [n.add_child(dist=float(rng.uniform(0.02, 0.3))) for n in level for _ in range(fan)]
    flat = FlatForest.from_trees([root])
    a, b, c = L_SHAPE
    assert flat.n_nodes == 1 + a + a * b + a * b * c + 2 * a * b * c and flat.n_tips == 2 * a * b * c
    return flat


def forest(k, which):
    return forest_s(k) if which == 'S' else forest_l()


@functools.lru_cache(maxsize=None)
def build(k, which, kind='EIGEN'):
    """dict(k, flat, specs [2], rates [2], masks [2, N, k])."""
    flat = forest(k, which)
    rng = np.random.default_rng(8000 + 2 * k + (which == 'L'))
    specs = [random_spec(kind, k, rng) for _ in range(2)]
    rates = [(float(rng.uniform(0.5, 3)), 0.0, 1.0), (float(rng.uniform(0.5, 3)), 0.01, 0.9)]
    observed = synthetic.one_hot_masks(flat, k, rng.integers(0, k, size=flat.n_tips))
    masks = np.stack([np.asarray(observed, dtype=np.int8), random_masks(flat, k, rng)])
    return dict(k=k, which=which, flat=flat, specs=specs, rates=rates, masks=masks)


@functools.lru_cache(maxsize=None)
def exact_pass(k, which, c, kind='EIGEN'):
    b = build(k, which, kind)
    return exact.marginal_pass(b['flat'], b['masks'][c], b['specs'][c], *b['rates'][c])


def oracle_as_logs(r):
    """An oracle result (full_marginal_pass) in the terms of the exact pass."""
    with np.errstate(divide='ignore'):
        return dict(bu_log10=np.log10(r['bu']) - r['bu_sf'][:, None], td_log10=np.log10(r['td']) - r['td_sf'][:, None],
                    lh_log10=np.log10(r['lh'].sum(axis=1)) - r['lh_sf'], posterior=r['posterior'], loglik=r['loglik'])


def errors(got, want):
    """
    got: dict(loglik (float), bu_log10, td_log10 [N, k], posterior [N, k], lh_log10 [N]) of the implementation under test, want: the
    exact pass.  Zero patterns of the vectors and posteriors must be equal (asserted).  Returns the worst errors, dict(
        lnl: |ln L - exact| / |exact|,  log10: the largest |difference| of a finite log10 entry of the two vectors,
        post: the largest |p - exact| / (exact + 1e-291) (rtol r on it is assert_allclose's rtol r with atol 1e-300 at r = 1e-9),
        lh: the largest relative error of a node's log10 likelihood sum).
    """
    out = dict(lnl=exact.rel_error(got['loglik'], want['loglik']))
    worst = 0.0
    for key in ('bu_log10', 'td_log10'):
        a, b = got[key], want[key]
        assert not np.isnan(b).any(), key
        assert np.array_equal(np.isneginf(a), np.isneginf(b)), key + ': zero patterns differ'
        fin = np.isfinite(b)
        worst = max(worst, float(np.abs(a[fin] - b[fin]).max()))
    out['log10'] = worst
    p, q = got['posterior'], want['posterior']
    assert np.all(np.isfinite(p)) and np.array_equal(p == 0, q == 0), 'posteriors: zero patterns differ'
    out['post'] = float((np.abs(p - q) / (q + 1e-291)).max())
    out['lh'] = float(np.abs(got['lh_log10'] / want['lh_log10'] - 1).max())
    return out


def ratios(err, k, lnl_rtol=LNL_RTOL, log10_tol=None, post_rtol=POST_RTOL):
    """error / tolerance per quantity."""
    return dict(lnl=err['lnl'] / lnl_rtol, log10=err['log10'] / (log10_tol or log10_atol(k)), post=err['post'] / post_rtol,
                lh=err['lh'] / lnl_rtol)


# ---------------------------------------------------------------------------------------------------------------------
# rescaling
# ---------------------------------------------------------------------------------------------------------------------
TIP_BRANCH, SPINE_BRANCH, END_BRANCH = 0.8, 0.05, 0.1   # (test_eigen_joint_sweep_wide_polytomies_and_deep_trees builds it so)
DEEP_LOG2 = -800.0
DEEP_RATES = (1.0, 0.02, 0.9)


@functools.lru_cache(maxsize=None)
def deep_caterpillar(kind, k):
    """
    dict(flat, spec, rates, masks [N, k], depth, spine (ids of the internal nodes from the root down), root_log2_exact): a caterpillar
    with one observed tip per level (tip branch 0.8, spine 0.05) and a cherry at its end.  Its depth is the smallest multiple of 50
    at which the exact bottom-up vector of the root has log2(max) below -800 -- four trips through the 2^+-200 band at least --,
    found by growing the caterpillar at the root end in exact arithmetic: level j from the end carries the j-th drawn state, so
    the deeper caterpillar contains the shallower one.
    """
    rng = np.random.default_rng(4300 + k)
    spec = random_spec(kind, k, rng)
    drawn = rng.integers(0, k, size=4000)
    with exact.decimal.localcontext(exact._CONTEXT):
        op = exact.operator(spec, [TIP_BRANCH, SPINE_BRANCH, END_BRANCH], *DEEP_RATES)

        def one_hot(s):
            v = np.array([exact.ZERO] * k, dtype=object)
            v[s] = exact.ONE
            return v
        tip_message = {}
        v = op.apply(2, one_hot(int(drawn[0]))) * op.apply(2, one_hot(int(drawn[1])))
        depth = 0
        while True:
            s = int(drawn[2 + depth])
            if s not in tip_message:
                tip_message[s] = op.apply(0, one_hot(s))
            v = tip_message[s] * op.apply(1, v)
            depth += 1
            root_log2 = exact.log10_float(max(v)) * exact.LOG2_OF_10
            if depth % 50 == 0 and root_log2 < DEEP_LOG2:
                break
    # the tree, from the root down: level d carries the state drawn for level depth - 1 - d from the end
    state_of = {}
    root = TreeNode(name='r', dist=0.0)
    cur = root
    spine_nodes = [root]
    for d in range(depth):
        state_of[id(cur.add_child(name='t{}'.format(d), dist=TIP_BRANCH))] = int(drawn[2 + depth - 1 - d])
        cur = cur.add_child(name='i{}'.format(d), dist=SPINE_BRANCH)
        spine_nodes.append(cur)
    state_of[id(cur.add_child(name='ta', dist=END_BRANCH))] = int(drawn[0])
    state_of[id(cur.add_child(name='tb', dist=END_BRANCH))] = int(drawn[1])
    flat = FlatForest.from_trees([root])
    masks = np.ones((flat.n_nodes, k), dtype=np.int8)
    index = {id(n): i for i, n in enumerate(flat.nodes)}
    for key, s in state_of.items():
        masks[index[key]] = 0
        masks[index[key], s] = 1
    return dict(flat=flat, spec=spec, rates=DEEP_RATES, masks=masks, depth=depth, spine=[index[id(n)] for n in spine_nodes],
                root_log2_exact=root_log2)


POLYTOMY_TREES = 140
POLYTOMY_BRANCH = 2.0
POLYTOMY_LOG2 = -230.0   # (aimed at; the test asserts -200 on the exact vectors)


@functools.lru_cache(maxsize=None)
def polytomy_forest(k):
    """
    dict(flat, spec, rates, masks, fan, polytomies (ids)): 140 trees, each a root with one child that is a polytomy of `fan` observed
    tips in the model's two rare states, on long branches.  The 140 polytomies are one level, wider than the narrow limit, so a
    LEVEL launch multiplies `fan` messages into one node: fan is chosen from the exact messages so that the product passes 2^-230.
    """
    rng = np.random.default_rng(5100 + k)
    # (random_spec with two rare states: on long branches a tip's message is about its state's frequency in every entry, and the
    # rarer the state the fewer tips it takes)
    pi = rng.dirichlet(np.ones(k) * 2)
    pi[:2] = 0.1 / k, 0.15 / k
    pi /= pi.sum()
    R = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
    d_, a_, ainv_ = orc.diagonalise(pi, R + R.T)
    spec = dict(kind=2, pi=pi, d=d_, A=a_, Ainv=ainv_)
    rates = (3.0, 0.0, 1.0)
    rare = [0, 1]
    with exact.decimal.localcontext(exact._CONTEXT):
        op = exact.operator(spec, [POLYTOMY_BRANCH], *rates)
        largest = exact.ZERO
        for s in rare:
            v = np.array([exact.ZERO] * k, dtype=object)
            v[s] = exact.ONE
            largest = max(largest, max(op.apply(0, v)))
        per_tip = exact.log10_float(largest) * exact.LOG2_OF_10
    assert per_tip < -1
    fan = int(np.ceil(POLYTOMY_LOG2 / per_tip))
    roots, state_of, polys = [], {}, []
    for _ in range(POLYTOMY_TREES):
        root = TreeNode(name='', dist=0.0)
        poly = root.add_child(dist=float(rng.uniform(0.05, 0.3)))
        polys.append(poly)
        for _t in range(fan):
            state_of[id(poly.add_child(dist=POLYTOMY_BRANCH))] = rare[int(rng.integers(2))]
        roots.append(root)
    flat = FlatForest.from_trees(roots)
    masks = np.ones((flat.n_nodes, k), dtype=np.int8)
    index = {id(n): i for i, n in enumerate(flat.nodes)}
    for key, s in state_of.items():
        masks[index[key]] = 0
        masks[index[key], s] = 1
    return dict(flat=flat, spec=spec, rates=rates, masks=masks, fan=fan, polytomies=np.array([index[id(n)] for n in polys]))


# ---------------------------------------------------------------------------------------------------------------------
# the joint (max-product) sweep: tests/test_gpu_joint_shapes.py, and the oracle in tests/test_matrix_exact_ref.py
# ---------------------------------------------------------------------------------------------------------------------
JOINT_WAVES = 4             # PML_WAVES_PER_BLOCK
JOINT_MIN_BLOCKS = 8        # launch_eigen_joint / launch_eigen_joint_tips: cap = max(8, EIGJ_BLOCKS / C)
J_TUNE = dict(EIGJ_BLOCKS=1, EIGJ_TIP_BLOCKS=1)
HKY_J_CHERRIES = 258        # above the plain narrow limit max(8, 512 / C) = 256 at two columns


def joint_narrow_limit(k):
    """Nodes per level up to which the joint sweep's levels next to the roots share one launch (pml_plan_bottom_up, BU_EIGJ)."""
    return JOINT_WAVES * (64 // k)


def j_cherries(k):
    """
    The width n of forest J(k)'s level of cherries.

    Up to 32 states, under J_TUNE: launch_eigen_joint takes blocks = min(ceil(n / (4 npw)), max(8, 1 / C)) = 8 workgroups of 4
    waves, and eigen_joint_kernel gives wave w the nodes [w npw + p stride, w npw + p stride + npw) in its pass p, with stride =
    32 npw.  With n = 64 npw + npw + 1 every wave makes two full passes (the prologue and one steady-state iteration that
    prefetches a third descriptor), wave 0 a third full pass (the nodes from 64 npw on), wave 1 a third pass of a single node,
    and the waves 2 .. 31 end after two (j_passes restates this arithmetic, and the device test asserts it).  n is odd where npw
    is even -- an even n leaves no partly filled wave at npw = 2 --, so the two halves of the forest differ by one cherry there.
    The tips kernels see 2 n tips: passes_total = ceil(2 n / npw) >= 130 over 32 waves, cp = min(ceil(passes_total / 32), 64 / npw)
    >= 2 passes per chunk (j_tip_chunk_passes).
    Beyond 32 states (one node per wave, the plain loop) 6 cherries with the default grid: two workgroups, the second one half idle.
    """
    if k > 32:
        return 6
    npw = 64 // k
    return 64 * npw + npw + 1


def j_tip_chunk_passes(k, n_tips, blocks_cap=JOINT_MIN_BLOCKS):
    """cp of eigen_joint_obs_tips_kernel / eigen_joint_tips_kernel: the passes a wave makes per chunk of tips."""
    npw = 64 // k
    blocks = min(-(-n_tips // (JOINT_WAVES * npw)), blocks_cap)
    passes_total = -(-n_tips // npw)
    return min(-(-passes_total // (blocks * JOINT_WAVES)), 64 // npw)


def j_passes(k, n):
    """(passes of wave 0, nodes in the last pass of the last wave that makes as many) of the level launch over n nodes under
    J_TUNE -- the arithmetic of launch_eigen_joint and eigen_joint_kernel restated."""
    npw = 64 // k
    blocks = min(-(-n // (JOINT_WAVES * npw)), JOINT_MIN_BLOCKS)
    stride = blocks * JOINT_WAVES * npw
    passes = -(-n // stride)
    left = n - (passes - 1) * stride          # nodes of the last pass, over the waves in order
    return passes, left - (-(-left // npw) - 1) * npw


@functools.lru_cache(maxsize=None)
def forest_j(n):
    """By hand, as forest L: a root, 2 children with n / 2 children each (rounded up and down), every one of those n a cherry of
    two tips.  Bottom-up the levels hold n, 2 and 1 nodes."""
    rng = np.random.default_rng(733 + n)

    def grow(nodes, fans):
        return [m.add_child(dist=float(rng.uniform(0.02, 0.3))) for m, fan in zip(nodes, fans) for _ in range(fan)]
    root = TreeNode(name='r', dist=0.0)
    halves = grow([root], [2])
    cherries = grow(halves, [n - n // 2, n // 2])
    grow(cherries, [2] * n)
    flat = FlatForest.from_trees([root])
    assert flat.n_nodes == 3 + 3 * n and flat.n_tips == 2 * n
    assert list(np.diff(flat.bu_offsets)) == [n, 2, 1]
    return flat


@functools.lru_cache(maxsize=None)
def forest_t():
    """((a,b),(c,d),e): two non-root internal nodes."""
    root = TreeNode(name='r', dist=0.0)
    for name, dist in (('ab', 0.11), ('cd', 0.07)):
        inner = root.add_child(name=name, dist=dist)
        inner.add_child(name=name[0], dist=0.19)
        inner.add_child(name=name[1], dist=0.05)
    root.add_child(name='e', dist=0.23)
    flat = FlatForest.from_trees([root])
    assert flat.n_nodes == 8 and flat.n_tips == 5
    return flat


@functools.lru_cache(maxsize=None)
def build_joint(k, which, kind='EIGEN'):
    """The inputs of a joint case, as build(): 'S' (build's own), 'J' (forest J(k); for HKY the J-shaped forest of 258 cherries),
    'T' (more than 64 states: every tip observed in column 0, one missing tip in column 1)."""
    if which == 'S':
        return build(k, 'S', kind)
    rng = np.random.default_rng(8600 + 2 * k + (which == 'T'))
    specs = [random_spec(kind, k, rng) for _ in range(2)]
    rates = [(float(rng.uniform(0.5, 3)), 0.0, 1.0), (float(rng.uniform(0.5, 3)), 0.01, 0.9)]
    if which == 'J':
        flat = forest_j(HKY_J_CHERRIES if kind == 'HKY' else j_cherries(k))
        observed = synthetic.one_hot_masks(flat, k, rng.integers(0, k, size=flat.n_tips))
        masks = np.stack([np.asarray(observed, dtype=np.int8), random_masks(flat, k, rng)])
    else:
        flat = forest_t()
        observed = np.asarray(synthetic.one_hot_masks(flat, k, rng.integers(0, k, size=flat.n_tips)), dtype=np.int8)
        missing = observed.copy()
        missing[flat.tips[int(rng.integers(flat.n_tips))]] = 1
        masks = np.stack([observed, missing])
    return dict(k=k, which=which, flat=flat, specs=specs, rates=rates, masks=masks)


@functools.lru_cache(maxsize=None)
def joint_exact(k, which, c, kind='EIGEN'):
    b = build_joint(k, which, kind)
    return exact.joint_pass(b['flat'], b['masks'][c], b['specs'][c], *b['rates'][c])


@functools.lru_cache(maxsize=None)
def deep_joint_exact(kind, k):
    d = deep_caterpillar(kind, k)
    return exact.joint_pass(d['flat'], d['masks'], d['spec'], *d['rates'])


@functools.lru_cache(maxsize=None)
def polytomy_joint_exact(k):
    d = polytomy_forest(k)
    return exact.joint_pass(d['flat'], d['masks'], d['spec'], *d['rates'])


def tree_sizes(flat):
    """Nodes per tree, in the order of flat.roots (parents have smaller ids than their children)."""
    root_of = np.arange(flat.n_nodes)
    for n in range(flat.n_nodes):
        if flat.parent[n] >= 0:
            root_of[n] = root_of[flat.parent[n]]
    return [int((root_of == r).sum()) for r in flat.roots]


def joint_errors(got, want, flat, masks, spec, rates):
    """
    got: dict(loglik (float), bu_log10 [N, k], table [N, k], states [N]) of the implementation under test, want: joint_pass.
    Asserts what has no tolerance to choose: equal zero patterns of the internal nodes' vectors, every table entry of every non-root
    node a maximum of the exact products up to products equal to 1e-12 (choice_is_a_maximum), every back-traced state allowed by its
    mask.  Returns the worst errors, dict(
        lnl: |ln L - exact| / |exact|,  log10: the largest |difference| of a finite log10 entry of an internal node's vector,
        scenario: the largest, over the trees, of (exact maximum - ln probability of the back-traced scenario) / nodes of the tree,
            in units of 1e-12: each choice within 1e-12 relative of its row's best puts the product within (1 + 1e-12)^n).
    """
    k = np.asarray(masks).shape[1]
    out = dict(lnl=exact.rel_error(got['loglik'], want['loglik']))
    inner = ~flat.is_tip
    a, b = got['bu_log10'][inner], want['bu_log10'][inner]
    assert not np.isnan(b).any()
    assert np.array_equal(np.isneginf(a), np.isneginf(b)), 'bottom-up vectors: zero patterns differ'
    fin = np.isfinite(b)
    out['log10'] = float(np.abs(a[fin] - b[fin]).max())
    for n in np.flatnonzero(flat.parent >= 0):
        for i in range(k):
            assert exact.choice_is_a_maximum(want['products'], int(n), i, int(got['table'][n, i])), ('table', int(n), i)
    states = np.asarray(got['states'])
    assert np.all((states >= 0) & (states < k)) and np.all(np.asarray(masks)[np.arange(flat.n_nodes), states] != 0), \
        'a back-traced state is not allowed by its mask'
    worst = 0.0
    for lp, best, size in zip(exact.scenario_log_probability(flat, masks, spec, *rates, states=states), want['loglik_per_tree'],
                              tree_sizes(flat)):
        assert lp.is_finite(), 'the back-traced scenario has probability zero'
        gap = float(best - lp)
        assert gap > -1e-40, 'a scenario above the exact maximum: {}'.format(gap)
        worst = max(worst, gap / size / 1e-12)
    out['scenario'] = worst
    return out


def oracle_joint(flat, masks, spec, rates):
    """The oracle's joint sweep and back-trace in the terms of joint_errors."""
    r = orc.bottom_up(flat, np.asarray(masks).astype(int), spec, *rates, is_marginal=False)
    with np.errstate(divide='ignore'):
        bu_log10 = np.log10(r['bu']) - r['bu_sf'][:, None]
    return dict(loglik=r['loglik'], bu_log10=bu_log10, table=r['joint_table'],
                states=orc.joint_backtrace(flat, r['bu'], r['joint_table'], spec['pi']))


@functools.lru_cache(maxsize=None)
def deep_exact(kind, k):
    d = deep_caterpillar(kind, k)
    return exact.marginal_pass(d['flat'], d['masks'], d['spec'], *d['rates'])


@functools.lru_cache(maxsize=None)
def polytomy_exact(k):
    d = polytomy_forest(k)
    return exact.marginal_pass(d['flat'], d['masks'], d['spec'], *d['rates'])
