"""The four observed tips of a two-level unit's child are finished in lanes (td_f81_super_unit).

The top-down two-level kernel runs the observed tips' closed form once per tip, in the lane that gathered the tip, where every
lane of the unit used to repeat it tip after tip; PASTML_HIP_NO_TIP_LANES is the off switch.  The results must be, bit for
bit, those of the one-by-one loop: every test here runs one engine as built and one with the switch on the same inputs, on
the level schedule with two-level units from the first node, and compares ln L and full downloads of the posteriors, the
likelihood sums and their exponents (as 64-bit words where NaNs are expected).  One column is tied to the oracle as well.
"""
import numpy as np
import pytest

from oracle import pastml_oracle as orc
from pastml_amd import hip, synthetic
from test_gpu_parity import LEVEL_SCHEDULE, LNL_RTOL, POST_RTOL, _forest_with_balanced_clumps, random_masks, random_spec
from test_gpu_tip_rows_kept import _observed_tip, _with_pi_s

pytestmark = pytest.mark.gpu

C = 3
SCHEDULE = dict(LEVEL_SCHEDULE, SMALL_MAX_NODES=0)   # (level launches however small the forest)
OFF = dict(NO_TIP_LANES=1)
FORESTS = ('balanced6', 'balanced12', 'clumps')


def forest_of(name):
    """64 tips (8 two-level nodes: one partially filled wave), 4096 tips, a ragged forest with balanced 8-tip clumps."""
    if name == 'balanced6':
        return synthetic.balanced_forest(6)
    if name == 'balanced12':
        return synthetic.balanced_forest(12)
    return _forest_with_balanced_clumps(700, seed=11)


def masks_of(flat, k, rng):
    """Column 0: every tip observed (the lanes path in every unit); column 1: unobserved and ambiguous tips among them (units
    with one to four tips that are not one-hot next to units of four observed tips, in one wave); column 2: observed tips
    below restricted internal nodes."""
    masks = np.empty((C, flat.n_nodes, k), dtype=np.int8)
    masks[0] = synthetic.one_hot_masks(flat, k, rng.integers(0, k, size=flat.n_tips))
    masks[1] = random_masks(flat, k, rng, missing=0.05, multi=0.05)
    masks[2] = random_masks(flat, k, rng, missing=0.0, multi=0.0, internal=0.05)
    return masks


def params_of(k, rng, n_passes=3):
    return [[(random_spec('F81', k, rng), (float(rng.uniform(0.4, 3)), 0.0, 1.0)) for _ in range(C)] for _ in range(n_passes)]


def tables(eng, lnl):
    return (np.array(lnl),) + tuple(np.stack([eng.download(what, c) for c in range(eng.n_cols)])
                                    for what in (hip.BUF_POSTERIOR, hip.BUF_LH_SUM, hip.BUF_LH_SF))


def one_pass(eng, models, check_launch=False):
    eng.set_models(models)
    if check_launch:
        eng.profile_enable(True)
    lnl, _, _, _ = eng.marginal_pass(posterior=False, lh=False)
    if check_launch:
        assert eng.profile_read(3)[1] > 0    # the two-level top-down launch ran
        eng.profile_enable(False)
    return tables(eng, lnl)


def same_bits(a, b):
    """Equal as 64-bit words (NaNs included)."""
    return len(a) == len(b) and all(
        x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))
        for x, y in zip(a, b))


def engines(flat, k, tune=SCHEDULE):
    on, off = hip.Engine(flat, C, k, tune=tune), hip.Engine(flat, C, k, tune=dict(tune, **OFF))
    for eng in (on, off):
        scheduled, n_two, _ = eng.schedule_info()
        assert scheduled and n_two > 0, (scheduled, n_two)
    return on, off


def three_passes(flat, k, tune, seed):
    """First pass (rows written), a second with other parameters (rows kept), a third with the rows left implicit: after
    each, the built engine's tables are the off-switch engine's.  Returns what the first pass used and gave."""
    rng = np.random.default_rng(seed)
    masks, params = masks_of(flat, k, rng), params_of(k, rng)
    on, off = engines(flat, k, tune)
    with on, off:
        on.set_masks(masks)
        off.set_masks(masks)
        first = None
        for i in range(3):
            if i == 2:
                on.set_option(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)
                off.set_option(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)
            got, want = one_pass(on, params[i], check_launch=i == 0), one_pass(off, params[i], check_launch=i == 0)
            assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all(), i
            for x, y in zip(got, want):
                assert np.array_equal(x, y), i
            first = first or got
    return masks, params[0], first


@pytest.mark.parametrize('k', [17, 20, 32, 40, 64])
@pytest.mark.parametrize('name', FORESTS)
def test_tips_in_lanes_give_the_bits_of_the_loop(name, k):
    """Lane shapes 8 x 4 (k <= 32) and 8 x 8, with padding states at k = 17, 20, 40; three forests; three kinds of masks;
    rows written, kept and implicit."""
    three_passes(forest_of(name), k, SCHEDULE, 100 * FORESTS.index(name) + k)


def test_tips_in_lanes_with_sixteen_lanes_per_unit():
    """BU_WIDE = 0 at k = 64: units of 16 lanes with four states each."""
    three_passes(forest_of('clumps'), 64, dict(SCHEDULE, BU_WIDE=0), 7)


def test_random_mask_column_matches_the_oracle():
    """Column 1 (observed, ambiguous and unobserved tips) of the first pass against the reference implementation."""
    flat, k = forest_of('clumps'), 20
    masks, models, got = three_passes(flat, k, SCHEDULE, 23)
    spec, rates = models[1]
    ref = orc.full_marginal_pass(flat, masks[1].astype(int), spec, *rates)
    np.testing.assert_allclose(got[0][1], ref['loglik'], rtol=LNL_RTOL)
    np.testing.assert_allclose(got[1][1], ref['posterior'], rtol=POST_RTOL, atol=1e-300)


def test_zero_frequencies():
    """pi_r = 0 at a state no tip of the column carries: prod_r = posterior_r x 0 in every unit, and the lanes path must give
    what the masked sum gave.  Then pi_s = 0 at a state observed tips of column 0 carry (c0 = (1 - e) pi_s = 0 for them,
    replaced by 1): that column's likelihood is zero at the root, no node vector is, so the pass returns; whatever it leaves
    in the tables, NaNs included, is what the off switch leaves, and the next good pass gives the off-switch engine's finite
    tables again."""
    k = 20
    flat = forest_of('balanced12')
    rng = np.random.default_rng(77)
    masks, params = masks_of(flat, k, rng), params_of(k, rng)
    nodes = np.arange(flat.n_nodes)
    unused = 5
    for c in range(C):   # no node is held to state `unused` (observed and restricted ones move on by one state, ambiguous ones lose it)
        carry = nodes[masks[c, nodes, unused] == 1]
        lone = carry[masks[c, carry].sum(axis=1) == 1]
        masks[c, lone, unused + 1] = 1
        multi = carry[masks[c, carry].sum(axis=1) < k]
        masks[c, multi, unused] = 0
    zero_unused = [_with_pi_s(params[0], c, unused, 0.0)[c] for c in range(C)]
    _, _, s = _observed_tip(flat, masks, 0)
    on, off = engines(flat, k)
    with on, off:
        on.set_masks(masks)
        off.set_masks(masks)
        got, want = one_pass(on, zero_unused, check_launch=True), one_pass(off, zero_unused, check_launch=True)
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
        assert same_bits(got, want)
        zero_observed = _with_pi_s(params[1], 0, s, 0.0)
        assert same_bits(one_pass(on, zero_observed), one_pass(off, zero_observed))
        got, want = one_pass(on, params[2]), one_pass(off, params[2])
        assert np.isfinite(want[1]).all() and same_bits(got, want)


@pytest.mark.parametrize('which', [0, 3])
def test_a_nan_row_takes_the_loop_and_is_repaired(which):
    """The construction of test_a_nan_row_is_repaired_by_the_next_good_pass (test_gpu_tip_rows_kept.py) on a tip of a two-level
    unit (that test's forest has none): one observed tip of column 1, the only one in its state s, on a branch of 1e-5 with
    pi_s = 1e-305 in the bad pass, so that lhs is not a positive finite number and the tip's row is NaNs.  On the 64-tip
    balanced tree the bad pass returns no error and a finite ln L (on 4096 tips, and on the forest with clumps, it raises the
    zero likelihood).  With the first observed tip of the column 126 rows of the column come out as NaNs (whole units whose
    P is not finite), with the fourth the tip's own row alone (one tip of a unit is not ok).  Either way the units fall back
    to the one-by-one loop: same bits as the off switch, NaNs and bad-tip word included, and the next good pass repairs the
    table."""
    k = 20
    flat = forest_of('balanced6')
    rng = np.random.default_rng(5)
    masks, params = masks_of(flat, k, rng), params_of(k, rng, 4)
    tips, tip, s = _observed_tip(flat, masks, 1, which)
    flat.dist[tip] = 1e-5
    others = [n for n in tips if n != tip and masks[1, n, s]]
    masks[1, others, s] = 0
    masks[1, others, (s + 1) % k] = 1
    on, off = engines(flat, k)
    with on, off:
        on.set_masks(masks)
        off.set_masks(masks)
        assert same_bits(one_pass(on, params[0], check_launch=True), one_pass(off, params[0], check_launch=True))
        bad = _with_pi_s(params[1], 1, s, 1e-305)
        got, want = one_pass(on, bad), one_pass(off, bad)
        assert np.isnan(want[1][1, tip]).all() and np.isfinite(want[1][[0, 2]]).all()
        assert same_bits(got, want)
        got = one_pass(on, params[2])
        assert same_bits(got, one_pass(off, params[2]))
        with hip.Engine(flat, C, k, tune=SCHEDULE) as fresh:
            fresh.set_masks(masks)
            assert same_bits(got, one_pass(fresh, params[2]))
        assert np.array_equal(got[1][1, tip], masks[1, tip].astype(float))
        assert same_bits(one_pass(on, params[3]), one_pass(off, params[3]))   # (rows kept again)
