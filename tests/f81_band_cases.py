"""
TEST INFRASTRUCTURE: inputs that drive the F81 units out of the rescaling band [2^-200, 2^200] where their shortcuts look, with
the exact results (tests/f81_exact_ref.py) computed once per process.  Host arithmetic only: tests/test_f81_band_cases_host.py
holds every case listed here to what tests/test_gpu_f81_band.py relies on, so that the GPU file filters nothing.

The shortcuts (pml_kernels_f81.h) skip lazy_rescale on a lower bound of a vector's non-zero entries: a cherry rebuilt from its
tips' lanes compares amin = prod over its tips of a = (1 - e)(pi . mask) with 2^-200 (2^-190 inside the two-level and top-down
units), a fast unit compares lob = prod over its children of a = (1 - e)(pi . v) with 2^-190.  With Dirichlet frequencies no
vector of a cherry, a pair unit or a two-level node comes near either, the skip is always taken and every exponent that travels
through LDS is 0.  Here the tips observe states whose frequency a bounded search has driven to its floor.

Forests (all scheduled with TUNE, the level schedule with units however small the forest):
    chained   synthetic.balanced_forest(7): 128 tips; PAIR units, 16 two-level nodes, 5 stacked nodes, both chains
    ragged    unit_schedule_cases.forest('ragged'): units, no chain, some three-child nodes
    fat       28 tips: root, 2, 4, 8 nodes, the last eight cherries of three and four tips in turn on branches with mu t' of 2e-5
              .. 1e-4 -- the body of the fast unit that is not PAIR.  The planner gives it the level schedule with one stacked node
              and no two-level unit (those take cherries of two tips), so it is a case of the plain level kernels and of the
              single-launch kernel; the GPU file asserts that this is what schedule_info() says
State counts: 20 (8 lanes x 4 states, padded), 32 (8 x 4), 33 (16 x 4 bottom-up, 8 x 8 top-down, padded) and 64 (8 x 8).  At 8 states
and fewer schedule_info() reports no units on these forests (measured on an MI355X at k = 8), so there is no such case.
Frequencies: three carrier states hold 0.5 / 0.3 / 0.2 of what the rare states leave (one carrier alone would send mu = 1 / (1 -
pi . pi) to infinity); every other state is rare and every observed tip is in a rare state.  Tiers of the
rare states' frequencies:
    bounds    10^-uniform(9, 12): where a bounded search ends; a two-level node's vector (8 tips) leaves the band
    pair      10^-uniform(19, 21): the vector leaves the band inside a PAIR unit (4 tips)
    cherry    10^-uniform(31, 36): amin < 2^-200 in a cherry of two tips
    straddle  three classes of rare states, 10^-(5.0 .. 5.3), 10^-(16.5 .. 16.8) and 10^-(37.5 .. 37.8) (fat: 10^-(4.0 .. 4.3) and
              10^-(8.0 .. 8.3) for the first two), one class per cherry and its tips in different states of it: over the nodes of
              height 1 the exact amin, and over those of height 2 and 3 the exact lob (above them a stored child has switched the
              bound off), fall on both sides of 2^-200 and 2^-190, and none lies within a factor 4 of either threshold (the host
              file asserts it on every column), so that rounding cannot move a unit across
Columns of a case: 0 every tip observed; 1 - 4 the four kinds of masks of test_gpu_td_chain.masks_of (observed; one tip in 20
unobserved; one in 20 ambiguous; internal nodes restricted), the states drawn among the rare ones; 5 as 0 with tau > 0 and
tau_factor < 1.  sf = 1.3.
"""
import decimal
import math

import numpy as np

import f81_exact_ref as exact
import unit_schedule_cases as units
from pastml_amd import synthetic
from pastml_amd.tree import FlatForest, TreeNode

TUNE = units.TUNE
KIND_F81 = 0
SF = 1.3
TAU, TAU_FACTOR = 0.011, 0.9
N_COLUMNS = 6
CONSUMER_COLUMNS = (0, 3, 5)   # the columns the consumers' exact references are computed for (a second per column at 64 states)
TIERS = dict(bounds=(9, 12), pair=(19, 21), cherry=(31, 36))
STRADDLE_CLASSES = dict(chained=((5.0, 5.3), (16.5, 16.8), (37.5, 37.8)), fat=((4.0, 4.3), (8.0, 8.3), (37.5, 37.8)))
# the draw of each straddle case: the first whose six columns keep the factor 4 (tests/test_f81_band_cases_host.py asserts it)
STRADDLE_DRAW = {('chained', 20): 0, ('chained', 32): 0, ('chained', 33): 0, ('chained', 64): 0, ('fat', 32): 0}
LOG2_BAND = 200          # lazy_rescale's band and the cherry's own check
LOG2_LOB = 190           # the fast units' check
MARGIN_LOG2 = 2          # a factor 4

CASES = [('chained', 'bounds', 20), ('chained', 'bounds', 32), ('chained', 'bounds', 33), ('chained', 'bounds', 64),
         ('chained', 'pair', 20), ('chained', 'pair', 33), ('chained', 'pair', 64),
         ('chained', 'cherry', 32), ('chained', 'cherry', 64),
         ('chained', 'straddle', 20), ('chained', 'straddle', 32), ('chained', 'straddle', 33), ('chained', 'straddle', 64),
         ('ragged', 'bounds', 20), ('ragged', 'bounds', 64), ('ragged', 'pair', 64), ('ragged', 'cherry', 20),
         ('fat', 'bounds', 20), ('fat', 'bounds', 33), ('fat', 'bounds', 64), ('fat', 'straddle', 32), ('fat', 'cherry', 20)]
IDS = ['{}-{}-{}'.format(*c) for c in CASES]

_forests = {}


def forest(name):
    if name not in _forests:
        if name == 'fat':
            rng = np.random.default_rng(2828)
            root = TreeNode(name='r', dist=0.0)
            level = [root]
            for _ in range(3):
                level = [n.add_child(dist=float(rng.uniform(0.02, 0.2))) for n in level for _c in range(2)]
            for i, cherry in enumerate(level):
                for _t in range(3 + i % 2):
                    cherry.add_child(dist=float(rng.uniform(1e-5, 5e-5)))
            _forests[name] = FlatForest.from_trees([root])
        elif name == 'chained':
            _forests[name] = synthetic.balanced_forest(7)
        else:
            _forests[name] = units.forest(name)
    return _forests[name]


def heights(flat):
    """[N]: 0 for a tip, 1 + the largest height of a child."""
    h = np.zeros(flat.n_nodes, dtype=np.int64)
    for n in reversed(range(flat.n_nodes)):
        p = int(flat.parent[n])
        if p >= 0:
            h[p] = max(h[p], h[n] + 1)
    return h


def _cherry_of_tip(flat):
    """Per tip (in tip order) the index of its parent among the tips' parents."""
    parents = flat.parent[flat.tips]
    _, index = np.unique(parents, return_inverse=True)
    return index


_built = {}


def build(name, tier, k):
    """dict(flat, pi [k], rare (the rare states), masks int8 [6, N, k], models: [(spec, (sf, tau, tf))] per column)."""
    key = (name, tier, k)
    if key in _built:
        return _built[key]
    assert key in CASES, key
    flat = forest(name)
    rng = np.random.default_rng(1000 * CASES.index(key) + k + 100000 * (STRADDLE_DRAW[name, k] if tier == 'straddle' else 0))
    carriers = np.sort(rng.choice(k, size=3, replace=False))
    rare = np.setdiff1d(np.arange(k), carriers)
    pi = np.zeros(k)
    tips = np.asarray(flat.tips)
    T = len(tips)
    if tier == 'straddle':
        # classes in turn over the rare states; the cherries of column c take the classes in turn from c on, so that the
        # class of a cherry, of its sibling and of its cousins all vary over a forest
        cls = np.arange(len(rare)) % 3
        for j, (lo, hi) in enumerate(STRADDLE_CLASSES[name]):
            pi[rare[cls == j]] = 10.0 ** -rng.uniform(lo, hi, size=int((cls == j).sum()))
        cherry = _cherry_of_tip(flat)
        pattern = np.array([0, 0, 1, 0, 2, 1, 1, 2, 0, 1, 2, 2, 0])

        def draw(c):
            # (the tips of a cherry in different states of its class: next to each other in a shuffled list)
            want = pattern[(cherry + c) % len(pattern)]
            lists = [rng.permutation(rare[cls == j]) for j in range(3)]
            place = np.zeros(T, dtype=np.int64)
            for ch in np.unique(cherry):
                place[cherry == ch] = np.arange(int((cherry == ch).sum())) + rng.integers(0, 64)
            return np.array([lists[w][i % len(lists[w])] for w, i in zip(want, place)])
    else:
        lo, hi = TIERS[tier]
        pi[rare] = 10.0 ** -rng.uniform(lo, hi, size=len(rare))

        def draw(c):
            return rng.choice(rare, size=T)
    pi[carriers] = np.array([0.5, 0.3, 0.2]) * (1.0 - pi[rare].sum())
    internal = np.flatnonzero(~flat.is_tip)
    masks = np.empty((N_COLUMNS, flat.n_nodes, k), dtype=np.int8)
    for c in range(N_COLUMNS):
        masks[c] = synthetic.one_hot_masks(flat, k, draw(c))
        some = tips[rng.random(T) < 0.05]
        if len(some) < 2:
            some = tips[[3, T // 2]]
        if c == 2:
            masks[c, some] = 1
        elif c == 3:
            for extra in range(2):
                masks[c, some[extra::2], rng.choice(rare, size=len(some[extra::2]))] = 1
        elif c == 4:
            held = internal[rng.random(len(internal)) < 0.02]
            if len(held) < 2:
                held = internal[[1, len(internal) // 2]]
            masks[c, held] = rng.random((len(held), k)) < 0.5
            masks[c, held, rng.choice(rare, size=len(held))] = 1
    masks.setflags(write=False)
    spec = dict(kind=KIND_F81, pi=pi)
    models = [(spec, (SF, 0.0, 1.0))] * (N_COLUMNS - 1) + [(spec, (SF, TAU, TAU_FACTOR))]
    _built[key] = dict(flat=flat, pi=pi, rare=rare, carriers=carriers, masks=masks, models=models, heights=heights(flat))
    return _built[key]


def _log2(x):
    """log2 of a positive Decimal as a float (-inf for 0): the decimal exponent plus the logarithm of the 17-digit mantissa, which
    is a hundred times faster than Decimal.log10 and exact to a few units of 2^-53 of the result."""
    if not x > 0:
        return -math.inf
    a = x.adjusted()
    return (a + math.log10(float(x.scaleb(-a)))) * LOG2_10


LOG2_10 = math.log2(10.0)
_exact = {}


def exact_pass(name, tier, k, c):
    """
    The exact marginal pass of column c, kept per process: dict(
        loglik (Decimal), G (Decimal), posterior [N, k] float,
        bu_log10, td_log10 [N, k] float: log10 of the exact vectors (-inf for zeros),
        lh_log10 [N]: log10 of every node's likelihood sum (its tree's likelihood),
        max_log2 [N]: log2 of the largest entry of the bottom-up vector; spread_log2 [N]: log2 of largest / smallest non-zero entry,
        lob_log2 [N]: log2 of prod over the node's children of a = (1 - e)(pi . v) (a cherry's amin; nan for tips)).
    """
    key = (name, tier, k, c)
    if key in _exact:
        return _exact[key]
    b = build(name, tier, k)
    flat = b['flat']
    spec, rates = b['models'][c]
    r = exact.marginal_pass(flat, b['masks'][c], b['pi'], *rates, top_down=True, vectors=False, raw=True)
    N = flat.n_nodes
    with decimal.localcontext(exact._CONTEXT):
        pi = [decimal.Decimal(float(x)) for x in b['pi']]
        bu = np.array([[_log2(x) for x in row] for row in r['v']])
        td = np.array([[_log2(x) for x in row] for row in r['down']])
        lob = np.full(N, np.nan)
        for n in range(N):
            fc, nc = int(flat.first_child[n]), int(flat.n_children[n])
            if nc:
                prod = exact.ONE
                for ch in range(fc, fc + nc):
                    prod *= (exact.ONE - r['e'][ch]) * exact._dot(pi, r['v'][ch])
                lob[n] = _log2(prod)
        lh = np.array([_log2(x) for x in r['lh']]) / LOG2_10
    with np.errstate(invalid='ignore'):
        finite = np.where(np.isfinite(bu), bu, np.nan)
        out = dict(loglik=r['loglik'], G=r['G'], posterior=r['posterior'], bu_log10=bu / LOG2_10, td_log10=td / LOG2_10,
                   lh_log10=lh, max_log2=np.nanmax(finite, axis=1), spread_log2=np.nanmax(finite, axis=1) - np.nanmin(finite, axis=1),
                   lob_log2=lob)
    _exact[key] = out
    return out


def _closest(got, want):
    """The largest |difference| of the finite entries of two log10 arrays with equal -inf patterns."""
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), 'zero patterns differ'
    fin = np.isfinite(want)
    return float(np.abs(got[fin] - want[fin]).max())


def errors(got, want, flat):
    """
    One column of an implementation under test -- dict(lnl, bu [N, k], bu_sf [N], td, td_sf, posterior [N, k], lh_sum [N], lh_sf [N])
    -- against exact_pass: error / tolerance per quantity, at the suite's tolerances.  ln L: LNL_RTOL |L| + 2^-53 G
    (f81_exact_ref.error_ratio); posteriors: POST_RTOL + 2 * 2^-53 * G relative, every non-zero entry, the same zeros; log10 of the
    true bottom-up vectors at internal nodes and of the top-down vectors at non-roots: LOG10_ATOL, the same zeros; log10 of every
    node's likelihood sum against its tree's exact likelihood: LH_RTOL relative.
    """
    from test_gpu_parity import LNL_RTOL, LOG10_ATOL, POST_RTOL, log_true
    inner, below = ~flat.is_tip, flat.parent >= 0
    out = dict(lnl=exact.error_ratio(got['lnl'], want, LNL_RTOL))
    post = got['posterior']
    assert np.isfinite(post).all()
    assert np.array_equal(post == 0, want['posterior'] == 0), 'posteriors: zero patterns differ'
    nz = want['posterior'] != 0
    rtol = POST_RTOL + 2 * float(exact.U53) * float(want['G'])
    out['post'] = float((np.abs(post[nz] - want['posterior'][nz]) / want['posterior'][nz]).max()) / rtol
    out['bu'] = _closest(log_true(got['bu'], got['bu_sf'])[inner], want['bu_log10'][inner]) / LOG10_ATOL
    out['td'] = _closest(log_true(got['td'], got['td_sf'])[below], want['td_log10'][below]) / LOG10_ATOL
    lh = np.log10(got['lh_sum']) - got['lh_sf']
    out['lh'] = float((np.abs(lh - want['lh_log10']) / np.abs(want['lh_log10'])).max()) / LH_RTOL
    return out


LH_RTOL = 1e-11
_joint = {}


def joint_exact(name, tier, k, c):
    key = (name, tier, k, c)
    if key not in _joint:
        b = build(name, tier, k)
        _joint[key] = exact.joint_pass(b['flat'], b['masks'][c], b['pi'], *b['models'][c][1])
    return _joint[key]
