"""
TEST INFRASTRUCTURE: the inputs on which the sum sweeps of the matrix models (eigen models, HKY) are held to exact arithmetic
(tests/matrix_exact_ref.py), shared by tests/test_matrix_exact_ref.py (the oracle, CPU) and tests/test_gpu_eigen_shapes.py (the
device).  Host arithmetic only.

For a state count k:

    forest S   some 60 nodes, up to four children per node, two trees, no zero-length branch: the tip launch and the
               several-levels-per-launch ("narrow") kernel.
    forest L   by hand: a root, 2 children, 4 children each, 17 children each, every one of those 136 a cherry of 2 tips
               (419 nodes).  Bottom-up the 136 cherries are one level above the narrow limit of the two-GEMM sweeps
               (2 x 4 waves x 16 = 128 nodes), the levels above (8, 2, 1) its narrow end; the 8 nodes of 17 children run the odd
               tail of the pair loop over children.  Top-down the depths hold 2, 8, 136 and 272 nodes: the first two are the
               narrow launch (a single narrow depth gets no launch of its own kind -- pml_schedule.cpp, narrow_levels -- which is
               why the 8 hang under 2 nodes and not under the root), the cherries and the tips a level launch each.
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


@functools.lru_cache(maxsize=None)
def deep_exact(kind, k):
    d = deep_caterpillar(kind, k)
    return exact.marginal_pass(d['flat'], d['masks'], d['spec'], *d['rates'])


@functools.lru_cache(maxsize=None)
def polytomy_exact(k):
    d = polytomy_forest(k)
    return exact.marginal_pass(d['flat'], d['masks'], d['spec'], *d['rates'])
