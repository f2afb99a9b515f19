"""
CPU tests of tests/f81_band_cases.py: what tests/test_gpu_f81_band.py relies on, so that it filters nothing and skips nothing.

For every case and column the exact ln L is finite, no posterior row is all zero, every non-zero exact posterior is above 1e-300
(so no entry is left out of a comparison), every vector's entry spread is below 2^400 (nothing underflows after a rescale), and
the oracle (float64, oracle/pastml_oracle.py) meets the tolerances the device is held to -- f81_band_cases.errors is the one
function both files use.  Per tier: which heights have vectors below 2^-200, where the cherries' amin and the units' lob lie, and
the straddle with its factor 4.
"""
import numpy as np
import pytest

import f81_band_cases as cases
from oracle import pastml_oracle as orc

BAND, LOB, MARGIN = cases.LOG2_BAND, cases.LOG2_LOB, cases.MARGIN_LOG2


def _columns(name, tier, k):
    return [cases.exact_pass(name, tier, k, c) for c in range(cases.N_COLUMNS)]


def test_the_list_of_cases():
    """About two dozen cases; the four lane shapes 20, 32, 33 and 64 on the chained forest at the bounds and the straddling tier;
    every forest at the bounds tier and at a tier that leaves the band below the two-level nodes."""
    assert 20 <= len(cases.CASES) <= 26 and len(set(cases.CASES)) == len(cases.CASES)
    for tier in ('bounds', 'straddle'):
        assert {k for name, t, k in cases.CASES if name == 'chained' and t == tier} >= {20, 32, 33, 64}
    for name in ('chained', 'ragged', 'fat'):
        assert {t for n, t, k in cases.CASES if n == name} >= {'bounds', 'cherry'}


def test_the_fat_forest():
    """root, 2, 4, 8: the eight cherries have three and four tips in turn, 28 tips."""
    flat = cases.forest('fat')
    h = cases.heights(flat)
    assert flat.n_tips == 28 and h.max() == 4 and (flat.n_children[h == 1] == [3, 4] * 4).all()
    assert (flat.n_children[h > 1] == 2).all() and [(h == x).sum() for x in (1, 2, 3, 4)] == [8, 4, 2, 1]


@pytest.mark.parametrize('name, tier, k', cases.CASES, ids=cases.IDS)
def test_every_column_is_usable_and_the_oracle_meets_the_tolerances(name, tier, k):
    b = cases.build(name, tier, k)
    flat, masks = b['flat'], b['masks']
    tips = flat.is_tip
    assert abs(b['pi'].sum() - 1) < 1e-15 and (b['pi'] > 0).all()
    assert masks.shape == (cases.N_COLUMNS, flat.n_nodes, k)
    for c in (0, 1, 5):   # every tip observed, in a rare state
        assert (masks[c][tips].sum(axis=1) == 1).all() and (masks[c][tips][:, b['carriers']] == 0).all()
    assert (masks[2][tips].sum(axis=1) == k).sum() >= 2                   # unobserved tips
    assert ((masks[3][tips].sum(axis=1) > 1) & (masks[3][tips].sum(axis=1) < k)).sum() >= 2   # ambiguous tips
    assert (masks[4][~tips].sum(axis=1) < k).sum() >= 2                   # restricted internal nodes
    assert b['models'][5][1][1] > 0 and b['models'][5][1][2] < 1
    worst = {}
    for c, want in enumerate(_columns(name, tier, k)):
        assert want['loglik'].is_finite()
        post = want['posterior']
        assert np.isfinite(post).all() and (post.sum(axis=1) > 0.999).all()
        assert post[post != 0].min() > 1e-300
        assert np.nanmax(want['spread_log2']) < 400
        spec, rates = b['models'][c]
        r = orc.full_marginal_pass(flat, masks[c].astype(int), spec, *rates)
        got = dict(lnl=r['loglik'], bu=r['bu'], bu_sf=r['bu_sf'], td=r['td'], td_sf=r['td_sf'], posterior=r['posterior'],
                   lh_sum=r['lh'].sum(axis=1), lh_sf=r['lh_sf'])
        e = cases.errors(got, want, flat)
        for q in e:
            worst[q] = max(worst.get(q, 0.0), e[q])
    print('f81-band oracle | {:8s} {:8s} k={:2d} | '.format(name, tier, k) + ' '.join('{} {:.3g}'.format(q, worst[q]) for q in sorted(worst)))
    assert max(worst.values()) < 1, worst


def _below(want, h, height):
    """(nodes of that height whose exact largest entry is below 2^-200, nodes of that height)"""
    sel = h == height
    return int((want['max_log2'][sel] < -BAND).sum()), int(sel.sum())


@pytest.mark.parametrize('name, tier, k', cases.CASES, ids=cases.IDS)
def test_the_claims_of_the_tier(name, tier, k):
    """
    bounds    no vector of height 1 or 2 is below 2^-200 (fat: of height 1); at least two in five of the two-level nodes' are, on the
              chained forest at k = 64 at least 14 of 16: the exponent into the chain is not zero
    pair      none of height 1; some of height 2 in every column; all of height 3
    cherry    every cherry of observed tips has amin < 2^-200 / 4; nine in ten of height 2 and all of height 3 are below 2^-200
    straddle  amin of the cherries on both sides of 2^-200, lob of the nodes of height 2 and 3 on both sides of 2^-190 (fat: over the
              columns together), and no amin or lob of these heights within a factor 4 of 2^-190 or 2^-200, in every column
    fat, bounds: over the columns some cherry of four tips has amin below 2^-200 and some above.
    """
    b = cases.build(name, tier, k)
    flat, h = b['flat'], b['heights']
    columns = _columns(name, tier, k)
    if tier == 'bounds':
        for want in columns:
            assert _below(want, h, 1)[0] == 0 and (name == 'fat' or _below(want, h, 2)[0] == 0)
            low, n = _below(want, h, 3)
            assert 5 * low >= 2 * n, (low, n)
            if (name, k) == ('chained', 64):
                assert low >= 14, low
        if name == 'fat':
            four = (h == 1) & (flat.n_children == 4)
            amin = np.concatenate([want['lob_log2'][four] for want in columns])
            assert (amin < -BAND - MARGIN).any() and (amin > -BAND + MARGIN).any()
    elif tier == 'pair':
        for want in columns:
            assert _below(want, h, 1)[0] == 0 and _below(want, h, 2)[0] > 0
            assert _below(want, h, 3)[0] == _below(want, h, 3)[1]
    elif tier == 'cherry':
        for c, want in enumerate(columns):
            if c in (0, 1, 5):
                assert (want['lob_log2'][h == 1] < -BAND - MARGIN).all()
            low, n = _below(want, h, 2)
            assert 10 * low >= 9 * n, (low, n)
            assert _below(want, h, 3)[0] == _below(want, h, 3)[1]
    else:
        for want in columns:
            amin, lob = want['lob_log2'][h == 1], want['lob_log2'][(h == 2) | (h == 3)]
            assert (amin > -BAND).any() and (amin < -BAND).any()
            assert name != 'chained' or ((lob > -LOB).any() and (lob < -LOB).any())
            both = np.concatenate((amin, lob))
            assert np.isfinite(both).all()
            for threshold in (BAND, LOB):
                assert (np.abs(both + threshold) > MARGIN).all(), both[np.abs(both + threshold) <= MARGIN]
        lob = np.concatenate([want['lob_log2'][(h == 2) | (h == 3)] for want in columns])
        assert (lob > -LOB).any() and (lob < -LOB).any()
    # (what test_rescaling_fired_where_it_must counts on, whatever the tier)
    height = dict(bounds=3, pair=2, cherry=2, straddle=2)[tier]
    for want in columns:
        assert _below(want, h, height)[0] > 0
        low_td = want['td_log10'].max(axis=1) * np.log2(10.0) < -BAND
        assert low_td[flat.is_tip].any()


# ---------------------------------------------------------------------------------------------------------------------
# the consumers of the pass on the bounds tier of the chained forest: float64 restatements of the sums of
# loglik_gradient_ref.py and expected_history_ref.py on the oracle's (rescaled) vectors and posteriors, held to the tolerances
# of tests/test_gpu_loglik_gradient.py and tests/test_gpu_expected_history.py -- a float64 implementation can meet them on
# these inputs, so tests/test_gpu_f81_band.py asks them of the device unchanged
# ---------------------------------------------------------------------------------------------------------------------

def _float64_branches(flat, masks, pi, sf, tau, tf):
    """Per non-root node, from the oracle's pass: (n, t', x = mu t', e, v_n (rescaled), S = pi . v_n, o = q_parent / message_n)."""
    r = orc.full_marginal_pass(flat, masks.astype(int), dict(kind=0, pi=pi), sf, tau, tf)
    mu = 1.0 / (1.0 - pi.dot(pi))
    out = []
    for n in np.flatnonzero(flat.parent >= 0):
        t = (flat.dist[n] + tau) * tf * sf
        e = np.exp(-mu * t)
        v = r['bu'][n]
        S = pi.dot(v)
        message = (1.0 - e) * S + e * v
        out.append((int(n), t, mu * t, e, v, S, r['posterior'][flat.parent[n]] / message))
    return r, mu, out


def _float64_gradient(flat, masks, pi, sf, tau, tf):
    r, mu, branches = _float64_branches(flat, masks, pi, sf, tau, tf)
    T0 = T1 = 0.0
    E = sum(r['bu'][root] / pi.dot(r['bu'][root]) for root in flat.roots)
    for n, t, x, e, v, S, o in branches:
        A, B = o.sum(), o.dot(v)
        h = -mu * e * (B - S * A)
        T0 += h
        T1 += h * t
        E = E + (1.0 - e) * A * v
    return np.array([T1 / sf, T0 * tf * sf, T1 / tf]), E + 2 * mu * pi * T1


def _float64_history(flat, masks, pi, sf, tau, tf):
    r, mu, branches = _float64_branches(flat, masks, pi, sf, tau, tf)
    k = len(pi)
    times, jumps, branch = np.zeros(k), np.zeros((k, k)), np.zeros(flat.n_nodes)
    for n, t, x, e, v, S, o in branches:
        g = -np.expm1(-x) / x
        c0, c1 = 1.0 - 2.0 * g + e, g - e
        O = o.sum()
        a = pi * O * S * c0 + o * S * c1
        b = pi * O * c1 + o * e
        times += (flat.dist[n] + tau) * tf * (a + b * v)
        jumps += x * pi[None, :] * (a[:, None] + b[:, None] * v[None, :])
        branch[n] = x * (a * (1.0 - pi) + b * (S - pi * v)).sum()
    np.fill_diagonal(jumps, 0.0)
    return times, jumps, branch


CONSUMERS = [c for c in cases.CASES if c[0] == 'chained' and c[1] == 'bounds']


@pytest.mark.parametrize('name, tier, k', CONSUMERS, ids=['{}-{}-{}'.format(*c) for c in CONSUMERS])
def test_float64_restatements_of_the_consumers_meet_their_tolerances(name, tier, k):
    import expected_history_ref as href
    import loglik_gradient_ref as gref
    import unit_schedule_cases as units
    from test_gpu_expected_history import TOLERANCE as HISTORY_TOLERANCE
    from test_gpu_loglik_gradient import TOLERANCE as GRADIENT_TOLERANCE
    b = cases.build(name, tier, k)
    flat = b['flat']
    worst = dict(gradient=0.0, history=0.0)
    for c in cases.CONSUMER_COLUMNS:
        spec, rates = b['models'][c]
        g = units.gradient(flat, b['masks'][c], spec['pi'], *rates)
        assert g['n_flat'] == 0
        d_rates, d_pi = _float64_gradient(flat, b['masks'][c], b['pi'], *rates)
        ratios = np.concatenate((gref.error_ratios(d_rates, [g['sf'], g['tau_fixed_tf'], g['tf']],
                                                   [g['gross_sf'], g['gross_tau_fixed_tf'], g['gross_tf']]),
                                 gref.error_ratios(d_pi, g['pi'], g['gross_pi'])))
        worst['gradient'] = max(worst['gradient'], ratios.max() / GRADIENT_TOLERANCE)
        h = units.history(flat, b['masks'][c], spec['pi'], *rates, jump_rows=None)
        times, jumps, branch = _float64_history(flat, b['masks'][c], b['pi'], *rates)
        ratio = max(href.relative_errors(times, h['times']).max(), href.relative_errors(branch, h['branch_jumps']).max(),
                    max(href.relative_errors(jumps[i], h['jumps'][i]).max() for i in range(k)))
        worst['history'] = max(worst['history'], ratio / HISTORY_TOLERANCE)
    print('f81-band float64 consumers | {:8s} {:8s} k={:2d} | gradient {:.3g} history {:.3g}'.format(name, tier, k, worst['gradient'],
                                                                                                worst['history']))
    assert worst['gradient'] < 1 and worst['history'] < 1, worst
