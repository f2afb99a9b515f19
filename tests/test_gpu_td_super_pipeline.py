"""The top-down two-level kernel loads one unit ahead (td_f81_super_issue / td_f81_super_unit).

The loads of unit i + 1 of a wave -- the two-level node's posterior row, sum and exponent, the child's four scalars, the gather
of the cherries' and tips' scalars -- are in flight while unit i is computed and stored; PASTML_HIP_NO_TD_SUPER_PIPE is the off
switch (the kernel instantiated with the loop that loads a unit's data when the unit begins).  The arithmetic is the same
statements on the same values, so every test here runs one engine as built and one with the switch on the same inputs, on the
level schedule with two-level units from the first node, and compares ln L and full downloads of the posteriors, the likelihood
sums and their exponents as 64-bit words, over three passes: rows written, rows kept, rows implicit.  Column 1 of the masks
(ambiguous and unobserved tips) sends units through the one-by-one loop over the tips, column 2 restricts internal nodes: both
run on prefetched data in every case.  One column is tied to the oracle as well.
"""
import numpy as np
import pytest

from oracle import pastml_oracle as orc
from pastml_amd import hip
from test_gpu_parity import LNL_RTOL, POST_RTOL
from test_gpu_tip_lanes import SCHEDULE, forest_of, masks_of, one_pass, params_of, same_bits

pytestmark = pytest.mark.gpu

C = 3
OFF = dict(NO_TD_SUPER_PIPE=1)
EIGHT_BLOCKS = dict(SCHEDULE, GRID_CAP=8)


def three_passes(flat, k, tune, seed):
    """First pass (rows written), a second with other parameters (rows kept), a third with the rows left implicit: after each,
    the built engine's tables are, word for word, the off-switch engine's.  Returns what the first pass used and gave."""
    rng = np.random.default_rng(seed)
    masks, params = masks_of(flat, k, rng), params_of(k, rng)
    on, off = hip.Engine(flat, C, k, tune=tune), hip.Engine(flat, C, k, tune=dict(tune, **OFF))
    with on, off:
        for eng in (on, off):
            scheduled, n_two, _ = eng.schedule_info()
            assert scheduled and n_two > 0, (scheduled, n_two)
            eng.set_masks(masks)
        first = None
        for i in range(3):
            if i == 2:
                on.set_option(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)
                off.set_option(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)
            got, want = one_pass(on, params[i], check_launch=True), one_pass(off, params[i], check_launch=True)
            assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all(), i
            assert same_bits(got, want), i
            first = first or got
    return masks, params[0], first


@pytest.mark.parametrize('k', [20, 64])
def test_prologue_and_tail_only(k):
    """64 tips: 16 units in one block.  Two waves run one iteration each, two waves have no unit at all: every load they
    issue is the clamped one of unit 0."""
    three_passes(forest_of('balanced6'), k, SCHEDULE, 600 + k)


@pytest.mark.parametrize('k', [17, 32, 64])
def test_four_iterations_per_wave(k):
    """4096 tips over 8 blocks: 1024 units, four per wave, so both buffers are used and the steady state is entered.  Lane
    shapes 8 x 4 (with padding states at k = 17) and 8 x 8."""
    three_passes(forest_of('balanced12'), k, EIGHT_BLOCKS, 1200 + k)


@pytest.mark.parametrize('k', [20, 64])
def test_ragged_unit_count(k):
    """Balanced 8-tip clumps in a ragged forest: the last wave pass is partly filled, and the units sit between nodes of the
    level launches."""
    three_passes(forest_of('clumps'), k, SCHEDULE, 700 + k)


def test_sixteen_lanes_per_unit():
    """BU_WIDE = 0 at k = 64: units of 16 lanes with four states each."""
    three_passes(forest_of('clumps'), 64, dict(SCHEDULE, BU_WIDE=0), 71)


def test_with_the_tips_finished_one_by_one():
    """NO_TIP_LANES in both engines: the kernel without the lanes path, with and without the prefetch."""
    three_passes(forest_of('balanced12'), 64, dict(EIGHT_BLOCKS, NO_TIP_LANES=1), 1299)


def test_random_mask_column_matches_the_oracle():
    """Column 1 (observed, ambiguous and unobserved tips) of the first pass against the reference implementation."""
    flat, k = forest_of('clumps'), 20
    masks, models, got = three_passes(flat, k, SCHEDULE, 29)
    spec, rates = models[1]
    ref = orc.full_marginal_pass(flat, masks[1].astype(int), spec, *rates)
    np.testing.assert_allclose(got[0][1], ref['loglik'], rtol=LNL_RTOL)
    np.testing.assert_allclose(got[1][1], ref['posterior'], rtol=POST_RTOL, atol=1e-300)
