"""
The exact selection reference (tests/select_states_ref.py) and the designed rows (tests/select_states_cases.py) on the host: what
tests/test_gpu_select_states.py relies on, so that it filters and skips nothing.

  * the reference's first minimiser of f(m) = (S - 2 L_m) / m is the first minimiser of the sum of squares the reference program
    writes (pastml/ml.py:546-560), evaluated in Fractions, and the identity between the two holds exactly;
  * ml.select_mppa / ml.select_map (float64) equal the exact reference on every decided row of every case, on the rows numpy
    computes as pi mask / sum; on the exact ties their answer is rounding and is printed, not asserted;
  * the census: every tier at every state count that admits it, sum = 0 rows at all seven lane shapes;
  * the dyadic rows are bit-identical to their designed values.
"""
from fractions import Fraction

import numpy as np
import pytest

import select_states_cases as cases
import select_states_ref as ref
from pastml_amd import ml


def masks_of(kept, k):
    out = np.zeros(k, dtype=np.int8)
    out[list(kept)] = 1
    return out


def exact_selection(lh, joint, method):
    """(masks [N, k], n_states [N], gaps [N]) of the exact reference on the doubles of lh."""
    N, k = lh.shape
    sel = np.zeros((N, k), dtype=np.int8)
    nsel = np.ones(N, dtype=np.int64)
    gaps = [None] * N
    for n in range(N):
        row = [float(x) for x in lh[n]]
        if method == 'MAP':
            sel[n, ref.select_map(row)] = 1
        else:
            r = ref.select_mppa(row, None if joint is None else int(joint[n]))
            sel[n] = masks_of(r['kept'], k)
            nsel[n] = r['m']
            gaps[n] = r['gap']
    return sel, nsel, gaps


def sample_rows():
    rng = np.random.default_rng(505)
    rows = [[Fraction(1, 2), Fraction(1, 4), Fraction(1, 8), Fraction(1, 8)], [Fraction(3, 4), Fraction(1, 4)],
            [Fraction(72, 100), Fraction(28, 100)], [Fraction(1, 5)] * 5, [Fraction(1, 2), 0, Fraction(1, 8), Fraction(1, 8)]]
    for k in (2, 3, 5, 8, 9):
        for _ in range(6):
            rows.append([Fraction(int(x)) for x in rng.integers(0, 12, size=k)])
    for k in (8, 9):
        b = cases.build(k, 'a')
        for c in range(b['C']):
            for n in range(0, min(b['N'], 40), 3):
                rows.append([Fraction(w * int(m)) for w, m in zip(b['weights'][c], b['masks'][c, n])])
    return [r for r in rows if sum(r) > 0]


def test_f_is_the_references_sum_of_squares():
    """sum (u_m - q)^2 = sum q^2 + (1 - 2 T_m) / m exactly, and the reference's first minimiser and gap are those of the sum."""
    rows = sample_rows()
    assert len(rows) > 60
    for row in rows:
        k = len(row)
        S = sum(row)
        sq = sum((x / S) ** 2 for x in row)
        for joint in [None] + list(range(k)):
            crit = ref.criterion_by_fractions(row, joint)
            f = ref.f_values(row, joint)
            assert [c - sq for c in crit] == f
            r = ref.select_mppa(row, joint)
            first = min(range(k), key=lambda m: (crit[m], m)) + 1
            assert r['m'] == first
            others = [crit[m] - crit[first - 1] for m in range(k) if m != first - 1]
            assert r['gap'] == (min(others) if others else None)
            order = sorted(range(k), key=lambda i: (-row[i], i))
            assert r['kept'] == sorted(order[:first])


def test_zero_row_and_map():
    assert ref.select_mppa([0.0] * 5, 2) == dict(m=5, gap=None, kept=[0, 1, 2, 3, 4], S=0)
    assert ref.select_map([0.0, 0.0]) == 0 and ref.select_map([0.1, 0.4, 0.4]) == 1


@pytest.mark.parametrize('k,part', cases.CASES, ids=['{}{}'.format(*c) for c in cases.CASES])
def test_host_restatement_equals_exact_reference(k, part):
    b = cases.build(k, part)
    post = cases.ideal_posteriors(b)
    for c in range(b['C']):
        if b['dyadic'][c]:
            assert np.array_equal(post[c], cases.designed_posteriors(b, c)), 'a dyadic row is not its designed value'
        for lh_on in (False, True):
            lh = post[c] * b['lh_masks'][c] if lh_on else post[c]
            want_map = np.array([ref.select_map(list(r)) for r in lh])
            assert np.array_equal(ml.select_map(lh).argmax(axis=1), want_map) and np.all(ml.select_map(lh).sum(axis=1) == 1)
            for fj in (False, True):
                joint = b['joint'][c] if fj else None
                sel, nsel, gaps = exact_selection(lh, joint, 'MPPA')
                designed = b['exact'][fj, lh_on][c]
                # the doubles decide as the designed integers do
                assert np.array_equal(nsel, [d['m'] for d in designed])
                assert np.array_equal(sel, [masks_of(d['kept'], k) for d in designed])
                kinds = np.array([d['kind'] for d in designed])
                for n in np.flatnonzero(kinds == 'decided'):
                    assert gaps[n] is None or gaps[n] >= cases.DECIDED
                for n in np.flatnonzero(kinds == 'tie'):
                    assert gaps[n] == 0
                with np.errstate(invalid='ignore', divide='ignore'):
                    host, host_k = ml.select_mppa(lh, joint)
                held = kinds != 'tie'
                assert np.array_equal(host_k[held], nsel[held]) and np.array_equal(host[held], sel[held])
    ties = cases.tie_answers(b)
    print('k = {} part {}: {} exact ties, ml.select_mppa differs from the first minimiser on (column, node, force_joint, lh_mask, '
          'template, its m, exact m): {}'.format(k, part, len(ties), [t for t in ties if t[5] != t[6]]))


@pytest.mark.parametrize('k', cases.STATE_COUNTS)
def test_census(k):
    census = cases.census_of(k)
    missing = cases.wanted(k) - {key for key, n in census.items() if n > 0}
    assert not missing, missing
    for part in cases.PARTS:
        b = cases.build(k, part)
        assert b['min_gap'] >= cases.DECIDED and b['N'] % 2 == 1
        assert all(d['kind'] in ('decided', 'tie', 'zero') for cfg in cases.CONFIGS for col in b['exact'][cfg] for d in col)


def test_zero_sums_at_every_lane_shape():
    shapes = {}
    for k in cases.STATE_COUNTS:
        shapes.setdefault(cases.lane_shape(k), []).append(cases.census_of(k)['scan'])
    assert sorted(shapes) == [(1, 8), (2, 8), (4, 8), (8, 8), (64, 2), (64, 4), (64, 8)]
    assert all(min(v) > 0 for v in shapes.values())
