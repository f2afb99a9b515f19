"""The chained top-down launch (td_f81_chain_kernel): the stacked units right above the two-level nodes run
inside the two-level launch and hand their grandchildren's rows to the two-level units through LDS.

The chained kernel runs td_f81_stack_unit and td_f81_super_unit on the values the two launches ran them on -- the row, sum and
exponent a two-level unit used to read back are, bit for bit, what the stacked unit has just stored -- so every test here runs one
engine as built and one with PASTML_HIP_NO_TD_CHAIN on the same inputs, both fresh, and compares ln L and full downloads of the
posteriors, the likelihood sums and their exponents (and the top-down vectors where kept) as 64-bit words.  The profile's
launch counts say whether the chain ran: one launch fewer in the top-down bracket than with the switch, the two-level bracket
used by both.  Columns cycle through four kinds of masks: every tip observed; some tips unobserved; some tips ambiguous (the
lanes path falls back); restricted internal nodes.  One column of a small forest is tied to exact arithmetic
(tests/f81_exact_ref.py) at the tolerance of test_gpu_optimiser_points.py.
"""
import numpy as np
import pytest

import f81_exact_ref as exact
from pastml_amd import hip, synthetic
from test_gpu_parity import LEVEL_SCHEDULE, LNL_RTOL, POST_RTOL, _forest_with_balanced_clumps, random_spec
from test_gpu_tip_rows_kept import _observed_tip, _with_pi_s

pytestmark = pytest.mark.gpu

OFF = dict(NO_TD_CHAIN=1)
SMALL = dict(LEVEL_SCHEDULE, SMALL_MAX_NODES=0)   # (level launches with two-level and stacked units however small the forest)
U53 = 2.0 ** -53
_FORESTS = {}


def forest(levels):
    if levels not in _FORESTS:
        _FORESTS[levels] = synthetic.balanced_forest(levels)
    return _FORESTS[levels]


def masks_of(flat, k, C, rng):
    """Column c: kind c % 4 -- 0 every tip observed, 1 one tip in 20 unobserved, 2 one tip in 20 ambiguous (two or three states),
    3 every tip observed and one internal node in 50 restricted to half of the states."""
    tips = np.flatnonzero(flat.is_tip)
    internal = np.flatnonzero(~flat.is_tip)
    masks = np.empty((C, flat.n_nodes, k), dtype=np.int8)
    for c in range(C):
        masks[c] = synthetic.one_hot_masks(flat, k, rng.integers(0, k, size=len(tips)))
        some = tips[rng.random(len(tips)) < 0.05]
        if c % 4 == 1:
            masks[c, some] = 1
        elif c % 4 == 2:
            for extra in range(2):
                masks[c, some[extra::2], rng.integers(0, k, size=len(some[extra::2]))] = 1
        elif c % 4 == 3:
            held = internal[rng.random(len(internal)) < 0.02]
            masks[c, held] = rng.random((len(held), k)) < 0.5
            masks[c, held, rng.integers(0, k, size=len(held))] = 1
    return masks


def params_of(k, C, rng, n_passes):
    return [[(random_spec('F81', k, rng), (float(rng.uniform(0.4, 3)), 0.0, 1.0)) for _ in range(C)] for _ in range(n_passes)]


def tables(eng, lnl, with_td):
    what = (hip.BUF_POSTERIOR, hip.BUF_LH_SUM, hip.BUF_LH_SF) + ((hip.BUF_TD, hip.BUF_TD_SF) if with_td else ())
    return (np.array(lnl),) + tuple(np.stack([eng.download(w, c) for c in range(eng.n_cols)]) for w in what)


def same_bits(a, b):
    """Equal as 64-bit words (NaNs included)."""
    return len(a) == len(b) and all(
        x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))
        for x, y in zip(a, b))


def one_pass(eng, models, with_td=False, counts=None):
    eng.set_models(models)
    if counts is not None:
        eng.profile_enable(True)
        for w in range(5):
            eng.profile_read(w, reset=True)
    lnl, _, _, _ = eng.marginal_pass(posterior=False, lh=False)
    if counts is not None:
        counts.append([eng.profile_read(w)[1] for w in range(5)])
        eng.profile_enable(False)
    return tables(eng, lnl, with_td)


def engines(flat, C, k, tune, keep_td=False, two_level=None, stacked=None):
    on, off = hip.Engine(flat, C, k, tune=tune, keep_td=keep_td), hip.Engine(flat, C, k, tune=dict(tune, **OFF), keep_td=keep_td)
    for eng in (on, off):
        scheduled, n_two, n_stacked = eng.schedule_info()
        assert scheduled and n_two > 0 and n_stacked > 0, (scheduled, n_two, n_stacked)
        assert two_level is None or n_two == two_level, n_two
        assert stacked is None or n_stacked == stacked, n_stacked
    return on, off


def chained(counts_on, counts_off):
    """The launch counts of a pass of each engine say that the chain ran: the stacked launch of one depth is gone from the
    top-down bracket, the two-level brackets are used as before, nothing else moved."""
    return (counts_on[1] == counts_off[1] - 1 and counts_on[3] == counts_off[3] == 1 and counts_on[4] == counts_off[4] == 1
            and counts_on[0] == counts_off[0] and counts_on[2] == counts_off[2])


def passes(flat, C, k, tune, seed, keep_td=False, two_level=None, stacked=None, expect_chain=True):
    """Rows written; other parameters, rows kept; a sweep of a column subset with new parameters, then the top-down sweep; the
    rows left implicit.  After each, the built engine's tables are the off-switch engine's.  Returns the first pass."""
    rng = np.random.default_rng(seed)
    masks, params = masks_of(flat, k, C, rng), params_of(k, C, rng, 4)
    on, off = engines(flat, C, k, tune, keep_td, two_level, stacked)
    with on, off:
        on.set_masks(masks)
        off.set_masks(masks)
        first = None
        for i in range(4):
            counts = ([], [])
            if i == 2:
                active = (np.arange(C) % 3 != 1).astype(np.uint8)
                got = []
                for eng in (on, off):
                    eng.set_models(params[i])
                    eng.bottom_up_submit(True, active=active)
                    lnl = np.asarray(eng.bottom_up_collect(True))
                    eng.top_down_marginals(posterior=False, lh=False)
                    got.append(tables(eng, lnl, keep_td))
                got, want = got
            else:
                if i == 3:
                    on.set_option(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)
                    off.set_option(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)
                got, want = one_pass(on, params[i], keep_td, counts[0]), one_pass(off, params[i], keep_td, counts[1])
                if expect_chain:
                    assert chained(counts[0][0], counts[1][0]), counts
                else:
                    assert counts[0] == counts[1] and counts[0][0][3] == 1, counts
            assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all(), i
            assert same_bits(got, want), i
            first = first or got
    return masks, params[0], first


@pytest.mark.parametrize('grid_cap', [None, 8])
def test_fifteen_levels_at_default_thresholds(grid_cap):
    """32 768 tips x 16 columns, k = 64 (8 lanes x 8 states): the level schedule with 4 096 two-level and 1 024 stacked nodes as
    the library picks it, 256 tiles.  As launched every wave has one tile; with GRID_CAP = 8 a wave walks eight tiles, so that
    the loads of a tile's first pass are issued in the tile before."""
    passes(forest(15), 16, 64, dict(GRID_CAP=grid_cap), 1500, two_level=4096, stacked=1024)


@pytest.mark.parametrize('k,wide,grid_cap', [(64, None, None), (64, None, 8), (32, None, None), (32, None, 8), (20, None, None),
                                             (64, 0, None), (64, 0, 8)])
def test_thirteen_levels(k, wide, grid_cap):
    """8 192 tips x 40 columns with STACK_MIN = 64: 1 024 two-level nodes below 256 stacked nodes; 64 tiles (128 with 16 lanes
    per unit, BU_WIDE = 0), the last the only tile of some waves; with GRID_CAP = 8 two or four tiles per wave.  Lane shapes 8 x
    8, 8 x 4 (with padding states at k = 20) and 16 x 4."""
    passes(forest(13), 40, k, dict(STACK_MIN=64, BU_WIDE=wide, GRID_CAP=grid_cap), 1300 + k, two_level=1024)


def test_top_down_vectors_kept():
    """PML_BUF_TD requested: both phases store the vectors and exponents of their nodes."""
    passes(forest(13), 40, 64, dict(STACK_MIN=64), 1364, keep_td=True)


@pytest.mark.parametrize('tune', [dict(NO_TIP_LANES=1), dict(NO_KEEP_TIP_ROWS=1), dict(NO_TD_SUPER_PIPE=1)])
def test_with_the_other_switches(tune):
    """The tips finished one by one and the rows written in every pass, chain on and off; without the pipeline the chain is
    off as well (it is the pipelined kernel's), and the launch counts say so."""
    passes(forest(9), 3, 64, dict(SMALL, **tune), 900, expect_chain='NO_TD_SUPER_PIPE' not in tune)


def test_a_ragged_forest_has_no_chain():
    """Balanced 8-tip clumps in a random forest: two-level and stacked units, but the lists do not line up -- the launches of
    the off switch, count for count."""
    passes(_forest_with_balanced_clumps(700, seed=11), 3, 20, SMALL, 700, expect_chain=False)


def test_a_nan_row_raises_the_bad_tip_word_and_is_repaired():
    """The construction of test_a_nan_row_takes_the_loop_and_is_repaired (test_gpu_tip_lanes.py) below the chained launch: one
    observed tip of column 0, the only one in its state s, on a branch of 1e-5 with pi_s = 1e-305 in the bad pass, so that its
    likelihood is zero and its row NaNs.  Same bits as the off switch, NaNs included; the next good pass, which must write
    every row again, repairs the table: the off-switch engine's and a fresh engine's."""
    k, C = 20, 3
    flat = synthetic.balanced_forest(6)
    rng = np.random.default_rng(5)
    masks, params = masks_of(flat, k, C, rng), params_of(k, C, rng, 4)
    tips, tip, s = _observed_tip(flat, masks, 0, 0)
    flat.dist[tip] = 1e-5
    others = [n for n in tips if n != tip and masks[0, n, s]]
    masks[0, others, s] = 0
    masks[0, others, (s + 1) % k] = 1
    on, off = engines(flat, C, k, SMALL)
    with on, off:
        on.set_masks(masks)
        off.set_masks(masks)
        counts = ([], [])
        assert same_bits(one_pass(on, params[0], counts=counts[0]), one_pass(off, params[0], counts=counts[1]))
        assert chained(counts[0][0], counts[1][0]), counts
        bad = _with_pi_s(params[1], 0, s, 1e-305)
        got, want = one_pass(on, bad), one_pass(off, bad)
        assert np.isnan(want[1][0, tip]).all() and np.isfinite(want[1][[1, 2]]).all()
        assert same_bits(got, want)
        got = one_pass(on, params[2])
        assert same_bits(got, one_pass(off, params[2]))
        with hip.Engine(flat, C, k, tune=SMALL) as fresh:
            fresh.set_masks(masks)
            assert same_bits(got, one_pass(fresh, params[2]))
        assert np.array_equal(got[1][0, tip], masks[0, tip].astype(float))
        assert same_bits(one_pass(on, params[3]), one_pass(off, params[3]))   # (rows kept again)


def test_against_exact_arithmetic():
    """512 tips, k = 20: ln L and the posteriors of the column with ambiguous and of the column with unobserved tips against
    exact arithmetic, at the tolerances of test_marginal_pass_at_the_optimisers_base_points."""
    flat, k, C = forest(9), 20, 3
    masks, models, got = passes(flat, C, k, SMALL, 909)
    for c in (1, 2):
        spec, rates = models[c]
        want = exact.marginal_pass(flat, masks[c], np.asarray(spec['pi']), *rates, top_down=True, vectors=False)
        assert exact.error_ratio(got[0][c], want, LNL_RTOL) < 1
        rtol = POST_RTOL + 2 * U53 * float(want['G'])
        assert np.array_equal(got[1][c] == 0, want['posterior'] == 0)
        big = want['posterior'] > 1e-300
        np.testing.assert_allclose(got[1][c][big], want['posterior'][big], rtol=rtol, atol=0)
