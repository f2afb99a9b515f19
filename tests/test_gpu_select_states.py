"""
select_states_kernel (pml_kernels_misc.h) against exact arithmetic on designed rows: every branch of the kernel -- the dominant-state
shortcut on both sides of 0.75 and 0.76, the candidate walk with its early stop right at m* and far behind it, the three ways of
writing the kept states, both tie rules, the reference-shaped scan of rows that sum to 0, at all seven lane shapes and every number
of mask words -- on forests of lone tips whose posterior rows tests/select_states_cases.py lays out (see there), compared with
tests/select_states_ref.py evaluated on the doubles the device itself delivers.

Per case (state count, part) one engine: a joint pass under one-hot masks names every row's joint state; then, for MAP and MPPA,
with and without force_joint and lh_masks, the designed masks are set, a marginal pass runs and the selection is compared:

  preconditions   the joint states are the designed ones; the dyadic rows arrive bit for bit; rows meant to sum to 0 under lh_masks do;
                  on the device's doubles every row is decided (gap >= 1e-10), tied (gap 0) or zero as designed.
  selection       masks and n_states equal the exact reference on EVERY row, as arrays; the decided rows also equal ml.select_mppa /
                  ml.select_map (on the exact ties the float64 restatement's answer is rounding: the kernel's contract there is
                  the first minimiser, which only the exact reference can name).
  as masks        bottom_up(True) right after the selection equals bottom_up(True) after set_masks(selected) bit for bit, and ln L
                  is sum_n ln sum_{i kept} pi_i to LNL_RTOL (with the floor of N sums' rounding where every tip keeps every state).

The capped runs (GRID_CAP = 8: eight workgroups per launch) walk the tips in several passes of the grid-stride loop, the last of
them with a partly filled wave (n >= N).
"""
import math

import numpy as np
import pytest

import select_states_cases as cases
from pastml_amd import hip, ml
from test_gpu_parity import LNL_RTOL
from test_select_states_ref import exact_selection, masks_of

pytestmark = pytest.mark.gpu

# (k, part, lone tips at least, tunables): every case as the library launches it, and five with a capped grid -- the tips are
# more than eight workgroups hold (4 waves of 64 / G tips each)
RUNS = [(k, part, None, None) for k, part in cases.CASES]
RUNS += [(2, 'a', 2101, dict(GRID_CAP=8)), (9, 'a', 1101, dict(GRID_CAP=8)), (64, 'a', 301, dict(GRID_CAP=8)),
         (65, 'a', None, dict(GRID_CAP=8)), (512, 'a', None, dict(GRID_CAP=8))]
METHODS = [('MAP', False, False), ('MAP', False, True), ('MPPA', False, False), ('MPPA', True, False), ('MPPA', False, True),
           ('MPPA', True, True)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.parametrize('k,part,n_min,tune', RUNS,
                         ids=['{}{}{}'.format(k, p, '-capped' if t else '') for k, p, _, t in RUNS])
def test_selection_equals_exact_reference(k, part, n_min, tune):
    b = cases.build(k, part, n_min)
    C, N, masks = b['C'], b['N'], b['masks']
    if tune:
        G = cases.lane_shape(k)[0]
        assert N > 8 * 4 * (64 // G), 'the capped grid covers every tip in one pass'
    with hip.Engine(b['flat'], C, k, tune=tune) as eng:
        eng.set_models(cases.specs_of(b))
        eng.set_masks(b['joint_masks'])
        eng.bottom_up(False)
        assert np.array_equal(eng.joint_backtrace(), b['joint']), 'the joint states are not the designed ones'
        first = None
        for method, fj, lh_on in METHODS:
            what = (method, fj, lh_on)
            eng.set_masks(masks)
            _, post, _, _ = eng.marginal_pass()
            if first is None:
                first = post
                for c in np.flatnonzero(b['dyadic']):
                    assert same_bits(post[c], cases.designed_posteriors(b, c)), 'a dyadic row did not arrive bit for bit'
                assert np.all(np.isfinite(post)) and np.all((post > 0) == (masks != 0))
            else:
                assert same_bits(post, first)
            sel, nsel = eng.select_states(method, force_joint=fj, lh_masks=b['lh_masks'] if lh_on else None)
            for c in range(C):
                lh = post[c] * b['lh_masks'][c] if lh_on else post[c]
                joint = b['joint'][c] if fj else None
                want, want_k, gaps = exact_selection(lh, joint, method)
                held = np.ones(N, dtype=bool)
                if method == 'MPPA':
                    designed = b['exact'][fj, lh_on][c]
                    kinds = np.array([d['kind'] for d in designed])
                    assert np.array_equal(lh.sum(axis=1) == 0, kinds == 'zero'), 'rows meant to sum to 0 (and only they) do'
                    for n in range(N):
                        if kinds[n] == 'decided':
                            assert gaps[n] is None or gaps[n] >= cases.DECIDED, (what, c, n, float(gaps[n]))
                        elif kinds[n] == 'tie':
                            assert gaps[n] == 0, (what, c, n, float(gaps[n]))
                    assert np.array_equal(want_k, [d['m'] for d in designed]), (what, c)
                    assert np.array_equal(want, [masks_of(d['kept'], k) for d in designed]), (what, c)
                    held = kinds != 'tie'
                    with np.errstate(invalid='ignore', divide='ignore'):
                        host, host_k = ml.select_mppa(lh, joint)
                else:
                    host, host_k = ml.select_map(lh), np.ones(N, dtype=np.int64)
                bad = np.flatnonzero((nsel[c] != want_k) | (sel[c] != want).any(axis=1))
                assert np.array_equal(nsel[c], want_k), (what, c, bad[:8], nsel[c][bad[:8]], want_k[bad[:8]])
                assert np.array_equal(sel[c], want), (what, c, bad[:8])
                assert np.array_equal(nsel[c][held], host_k[held]) and np.array_equal(sel[c][held], host[held]), (what, c)
            # the selection became the columns' masks
            lnl = eng.bottom_up(True)
            eng.set_masks(sel)
            assert same_bits(lnl, eng.bottom_up(True)), (what, 'the masks on the device are not the selection')
            # (a tip that keeps every state has the likelihood sum_i pi_i: 1 up to the rounding of a sum of k doubles, at most (k - 1)
            # 2^-53 in whatever order -- where all N tips of a column do, ln L is that rounding, and no relative bound on it means
            # anything: the floor is the N sums' worst case, as tests/degenerate_forest_cases.py holds its trees without information)
            for c in range(C):
                kept = [math.fsum(b['pi'][c][sel[c, n] != 0]) for n in range(N)]
                np.testing.assert_allclose(lnl[c], math.fsum(math.log(x) for x in kept), rtol=LNL_RTOL, atol=N * k * 2.0 ** -53,
                                           err_msg=str(what))
