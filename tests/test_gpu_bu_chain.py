"""The chained bottom-up launch (bu_f81_chain_kernel): the stacked units of the lowest stacked level run inside
the two-level launch and take their grandchildren's vectors, pi . v and exponents from LDS.

The chained kernel runs bu_f81_super_unit and bu_f81_stack_unit on the values the two launches ran them on -- what a stacked unit
used to read back is, bit for bit, what the two-level unit has just stored -- so every test here runs one engine as built and one
with PASTML_HIP_NO_BU_CHAIN on the same inputs, both fresh, and compares as 64-bit words: ln L, full downloads of the bottom-up
vectors and their exponents, and posteriors, likelihood sums and exponents after the top-down sweep.  The profile's launch counts
say whether the chain ran: one launch fewer in the bottom-up bracket than with the switch, the two-level brackets used once by
both.  Columns cycle through the four kinds of masks of test_gpu_td_chain.py.  One column of a small forest is tied to exact
arithmetic (tests/f81_exact_ref.py) at the tolerances of test_gpu_td_chain.py::test_against_exact_arithmetic.
"""
import numpy as np
import pytest

import f81_exact_ref as exact
from pastml_amd import hip
from pastml_amd.tree import FlatForest
from test_gpu_parity import LEVEL_SCHEDULE, LNL_RTOL, POST_RTOL, _forest_with_balanced_clumps
from test_gpu_td_chain import forest, masks_of, params_of, same_bits

pytestmark = pytest.mark.gpu

OFF = dict(NO_BU_CHAIN=1)
SMALL = dict(LEVEL_SCHEDULE, SMALL_MAX_NODES=0)   # (level launches with two-level and stacked units however small the forest)
U53 = 2.0 ** -53
BOTH_SWEEPS = (hip.BUF_BU, hip.BUF_BU_SF, hip.BUF_POSTERIOR, hip.BUF_LH_SUM, hip.BUF_LH_SF)


def tables(eng, lnl, what=BOTH_SWEEPS):
    return (np.array(lnl),) + tuple(np.stack([eng.download(w, c) for c in range(eng.n_cols)]) for w in what)


def counted(eng, run):
    """run() under the profile: its result and the launches of the five brackets."""
    eng.profile_enable(True)
    for w in range(5):
        eng.profile_read(w, reset=True)
    out = run()
    counts = [eng.profile_read(w)[1] for w in range(5)]
    eng.profile_enable(False)
    return out, counts


def one_pass(eng, models, counts=None):
    eng.set_models(models)
    if counts is None:
        lnl = eng.marginal_pass(posterior=False, lh=False)[0]
    else:
        lnl, got = counted(eng, lambda: eng.marginal_pass(posterior=False, lh=False)[0])
        counts.append(got)
    return tables(eng, lnl)


def engines(flat, C, k, tune, two_level=None, stacked=None):
    on, off = hip.Engine(flat, C, k, tune=tune), hip.Engine(flat, C, k, tune=dict(tune, **OFF))
    for eng in (on, off):
        scheduled, n_two, n_stacked = eng.schedule_info()
        assert scheduled and n_two > 0 and n_stacked > 0, (scheduled, n_two, n_stacked)
        assert two_level is None or n_two == two_level, n_two
        assert stacked is None or n_stacked == stacked, n_stacked
    return on, off


def chained(counts_on, counts_off):
    """The launch counts of a pass of each engine say that the chain ran: the stacked launch of one level is gone from the
    bottom-up bracket, the two-level brackets are used once as before, nothing else moved."""
    return (counts_on[0] == counts_off[0] - 1 and counts_on[4] == counts_off[4] == 1 and counts_on[3] == counts_off[3] == 1
            and counts_on[1] == counts_off[1] and counts_on[2] == counts_off[2])


def first_pass(flat, C, k, tune, seed, two_level=None, stacked=None, expect_chain=True):
    """One marginal pass of each engine on the four kinds of masks: the launch counts, then every table."""
    rng = np.random.default_rng(seed)
    masks, params = masks_of(flat, k, C, rng), params_of(k, C, rng, 1)
    on, off = engines(flat, C, k, tune, two_level, stacked)
    with on, off:
        on.set_masks(masks)
        off.set_masks(masks)
        counts = ([], [])
        got, want = one_pass(on, params[0], counts[0]), one_pass(off, params[0], counts[1])
        if expect_chain:
            assert chained(counts[0][0], counts[1][0]), counts
        else:
            assert counts[0] == counts[1] and counts[0][0][4] == 1, counts
        assert all(np.isfinite(t).all() for t in want)
        assert same_bits(got, want)
    return masks, params[0], got


@pytest.mark.parametrize('grid_cap', [None, 8])
def test_fifteen_levels_at_default_thresholds(grid_cap):
    """32 768 tips x 16 columns, k = 64 (8 lanes x 8 states): the level schedule with 4 096 two-level and 1 024 stacked nodes of
    the chained level as the library picks it, 128 tiles.  As launched every wave has one tile; with GRID_CAP = 8 a wave walks
    eight tiles, so that the loads of a tile's first pass are issued in the tile before."""
    first_pass(forest(15), 16, 64, dict(GRID_CAP=grid_cap), 1500, two_level=4096, stacked=1024)


@pytest.mark.parametrize('k,wide,grid_cap', [(64, None, None), (64, None, 8), (32, None, None), (32, None, 8), (20, None, None),
                                             (20, None, 8), (64, 0, None), (64, 0, 8)])
def test_thirteen_levels(k, wide, grid_cap):
    """8 192 tips x 40 columns with STACK_MIN = 64: 1 024 two-level nodes below 256 stacked nodes; 32 tiles (64 with 16 lanes
    per unit, BU_WIDE = 0); with GRID_CAP = 8 two or four tiles per wave.  Lane shapes 8 x 8, 8 x 4 (with padding states at k =
    20) and 16 x 4."""
    first_pass(forest(13), 40, k, dict(STACK_MIN=64, BU_WIDE=wide, GRID_CAP=grid_cap), 1300 + k, two_level=1024)


def test_a_part_filled_tile():
    """128 tips: 16 two-level nodes below the 4 stacked nodes of the chained level (and the root, stacked on its own level) --
    half a wave pass of stacked units, two of the tile's four two-level passes empty."""
    first_pass(forest(7), 3, 64, SMALL, 700, two_level=16, stacked=5)


def test_a_sequence_of_passes():
    """On one pair of engines: a pass; new parameters; a sweep of a column subset followed by the top-down sweep; the tips'
    rows left implicit; and the same pass again, which replays the captured graph."""
    flat, C, k = forest(11), 5, 64
    rng = np.random.default_rng(1100)
    masks, params = masks_of(flat, k, C, rng), params_of(k, C, rng, 4)
    on, off = engines(flat, C, k, dict(SMALL, STACK_MIN=16), two_level=256)
    with on, off:
        on.set_masks(masks)
        off.set_masks(masks)
        counts = ([], [])
        assert same_bits(one_pass(on, params[0], counts[0]), one_pass(off, params[0], counts[1]))
        assert chained(counts[0][0], counts[1][0]), counts
        assert same_bits(one_pass(on, params[1]), one_pass(off, params[1]))
        active = (np.arange(C) % 3 != 1).astype(np.uint8)
        got = []
        for eng in (on, off):
            eng.set_models(params[2])
            eng.bottom_up_submit(True, active=active)
            lnl = np.asarray(eng.bottom_up_collect(True))
            eng.top_down_marginals(posterior=False, lh=False)
            got.append(tables(eng, lnl))
        assert np.isfinite(got[1][0]).all() and same_bits(*got)
        for eng in (on, off):
            eng.set_option(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)
        again = []
        for _ in range(2):   # (the second one is the replay)
            got, want = one_pass(on, params[3]), one_pass(off, params[3])
            assert same_bits(got, want)
            again.append(got)
        assert same_bits(*again)


@pytest.mark.parametrize('tune', [dict(NO_TD_CHAIN=1), dict(NO_TD_SUPER_PIPE=1), dict(NO_TIP_LANES=1), {}])
def test_with_the_other_switches(tune):
    """The top-down chain, the top-down pipeline and the tips in lanes, each off and (the last case) all on: the bottom-up chain
    runs either way."""
    first_pass(forest(9), 3, 64, dict(SMALL, **tune), 900)


def test_a_ragged_forest_has_no_chain():
    """Balanced 8-tip clumps in a random forest: two-level and stacked units, but the lists do not line up -- the launches of
    the off switch, count for count."""
    first_pass(_forest_with_balanced_clumps(700, seed=11), 3, 20, SMALL, 701, expect_chain=False)


def _failing_pass(eng, models):
    eng.set_models(models)
    with pytest.raises(hip.ZeroLikelihoodError) as e:
        eng.bottom_up(True)
    err = e.value
    return np.array(err.loglik), np.array(err.err_parent, dtype=np.float64), np.array(err.err_child, dtype=np.float64)


def test_all_zero_vectors_take_the_sequential_path():
    """Column 1: a child of a two-level node with an empty mask -- the zero shows inside a two-level unit, which repeats on the
    sequential path, and its tile runs the stacked units on memory.  Column 2: the two children of a stacked node of the
    chained level on branches of length zero and restricted to disjoint halves of the states, whatever the tips say -- every
    two-level unit is fine and the zero shows first at the stacked node, whose unit repeats on the sequential path.  ln L and
    the pair each report names are the off switch's (the library serves no table after a sweep that reported a zero
    likelihood); columns 0 and 3 get the ln L they get without the bad columns; the next good pass, every table of it, equals
    the off switch's and a fresh engine's."""
    k, C, levels = 64, 4, 9
    flat = forest(levels)
    first = lambda depth: 2 ** depth - 1   # (breadth-first ids: the nodes of a depth are a contiguous range)
    stacked_node = first(levels - 5) + 5
    kids = [int(flat.first_child[stacked_node]), int(flat.first_child[stacked_node]) + 1]
    assert flat.parent[flat.first_child[flat.first_child[kids[0]]]] == flat.first_child[kids[0]]
    dist = np.array(flat.dist)
    dist[kids] = 0.0
    flat = FlatForest(flat.parent, flat.n_children, flat.first_child, dist, flat.roots)
    rng = np.random.default_rng(909)
    good, params = masks_of(flat, k, C, rng), params_of(k, C, rng, 2)
    bad = good.copy()
    two_level_child = first(levels - 2) + 77
    bad[1, two_level_child] = 0
    bad[2, kids[0]] = np.arange(k) < k // 2
    bad[2, kids[1]] = np.arange(k) >= k // 2
    on, off = engines(flat, C, k, SMALL, two_level=64)
    with on, off, hip.Engine(flat, C, k, tune=SMALL) as fresh:
        for eng in (on, off):
            eng.set_masks(bad)
        got, want = _failing_pass(on, params[0]), _failing_pass(off, params[0])
        assert want[1][0] == want[1][3] == -1 and want[1][1] == two_level_child and want[1][2] == stacked_node, want[1:]
        assert want[2][2] == kids[1], want[1:]
        assert np.isfinite(want[0][[0, 3]]).all() and not np.isfinite(want[0][[1, 2]]).any()
        assert same_bits(got, want)
        fresh.set_masks(good)
        clean = one_pass(fresh, params[0])
        assert same_bits([got[0][[0, 3]]], [clean[0][[0, 3]]])
        for eng in (on, off):
            eng.set_masks(good)
        got = one_pass(on, params[1])
        assert same_bits(got, one_pass(off, params[1]))
        assert same_bits(got, one_pass(fresh, params[1]))


def test_the_joint_sweep_is_unchanged():
    """The joint sweep (bottom_up(False) and joint_pass) on a context whose marginal sweep chains: the same launches and the same
    bits as with the switch."""
    flat, C, k = forest(9), 3, 64
    rng = np.random.default_rng(990)
    masks, params = masks_of(flat, k, C, rng), params_of(k, C, rng, 1)
    on, off = engines(flat, C, k, SMALL)
    with on, off:
        got = []
        for eng in (on, off):
            eng.set_masks(masks)
            marginal = one_pass(eng, params[0])
            lnl, c1 = counted(eng, lambda: eng.bottom_up(False))
            joint, c2 = counted(eng, lambda: eng.joint_pass())
            got.append((marginal + (np.array(lnl), np.array(joint[0]), np.asarray(joint[1]).astype(np.float64)), c1, c2))
        assert got[0][1:] == got[1][1:], (got[0][1:], got[1][1:])
        assert same_bits(got[0][0], got[1][0])


def test_against_exact_arithmetic():
    """512 tips, k = 20: ln L and the posteriors of the column with unobserved and of the column with ambiguous tips against exact
    arithmetic, at the tolerances of test_gpu_td_chain.py::test_against_exact_arithmetic."""
    flat, k, C = forest(9), 20, 3
    masks, models, got = first_pass(flat, C, k, SMALL, 909)
    for c in (1, 2):
        spec, rates = models[c]
        want = exact.marginal_pass(flat, masks[c], np.asarray(spec['pi']), *rates, top_down=True, vectors=False)
        assert exact.error_ratio(got[0][c], want, LNL_RTOL) < 1
        rtol = POST_RTOL + 2 * U53 * float(want['G'])
        assert np.array_equal(got[3][c] == 0, want['posterior'] == 0)
        big = want['posterior'] > 1e-300
        np.testing.assert_allclose(got[3][c][big], want['posterior'][big], rtol=rtol, atol=0)
