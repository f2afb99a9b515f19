"""
GPU tests (``-m gpu``) of the F81 units where their vectors leave the rescaling band: the band shortcuts of
f81_cherry_from_lanes, bu_f81_marg_body and its copies in the two-level and stacked units and of the top-down units, the
exponents that travel with the vectors through LDS (bu_chain_slot_store -> BuKidsOfChain, TdRowToLds) and the exponent arithmetic
of f81_finish_child and f81_tip_closed_form -- against exact arithmetic (tests/f81_exact_ref.py) on the inputs of
tests/f81_band_cases.py, where rare states' frequencies of 1e-9 down to 1e-36 put the vectors of cherries, pair units and
two-level nodes below 2^-200.  tests/test_f81_band_cases_host.py holds every case to a finite ln L, non-zero exact posteriors
above 1e-300 and the claims of each tier, and the oracle to the tolerances used here, so nothing is filtered or skipped.

Every case runs under four schedules, each on a fresh context that keeps its top-down vectors: the level schedule with units
(test_gpu_bu_chain.SMALL), the same without the bottom-up chain, the same without the top-down chain, and the library's own choice
for so small a forest.  schedule_info(), sweep_schedule() and the profile's launch counts say which ran (SCHEDULES, _assert_ran).

    exact values    ln L at LNL_RTOL |L| + 2^-53 G (f81_exact_ref.error_ratio); posteriors at POST_RTOL + 2 * 2^-53 * G with the same
                    zeros; log10 of the true bottom-up vectors at internal nodes and of the top-down vectors at non-roots at
                    LOG10_ATOL, the same zeros; log10 of every node's likelihood sum against the tree's exact ln L / ln 10 at 1e-11
    rescaling       BU_SF != 0 wherever the exact vector's largest entry is below 2^-200, TD_SF != 0 likewise
    soundness       every stored internal bottom-up vector has all non-zero entries in [2^-200, 2^200] or its maximum in [1, 2)
                    (pml_device.h, "lazy rescaling band"), whatever the schedule: a skipped rescale that was due shows here
    chains          with and without each chain: ln L, vectors, exponents, posteriors, sums and their exponents as 64-bit words
    joint sweep     bottom_up(False) on the bounds and pair tiers against f81_exact_ref.joint_pass
    consumers       loglik_gradient and expected_history on the bounds tier of the chained forest, by their own tests' checkers

Every case prints its worst error / tolerance per schedule ('f81-band | ...', pytest -s); profiles/f81_band_exact.txt holds those
lines from an MI355X.
"""
import numpy as np
import pytest

import expected_history_ref as href
import f81_band_cases as cases
import f81_exact_ref as exact
import test_gpu_bu_chain as bu_chain
import test_gpu_expected_history as thistory
import test_gpu_loglik_gradient as tgradient
import test_gpu_td_chain as td_chain
import unit_schedule_cases as units
from pastml_amd import hip
from test_gpu_parity import LEVEL_SCHEDULE, LNL_RTOL

pytestmark = pytest.mark.gpu

SMALL = dict(LEVEL_SCHEDULE, SMALL_MAX_NODES=0)
assert SMALL == cases.TUNE
# name -> tune (None: the library's own schedule)
SCHEDULES = dict(units=SMALL, no_bu_chain=dict(SMALL, NO_BU_CHAIN=1), no_td_chain=dict(SMALL, NO_TD_CHAIN=1), default=None)
LOG2_10 = float(np.log2(10.0))
TABLES = (hip.BUF_BU, hip.BUF_BU_SF, hip.BUF_TD, hip.BUF_TD_SF, hip.BUF_POSTERIOR, hip.BUF_LH_SUM, hip.BUF_LH_SF)
NAMES = ('bu', 'bu_sf', 'td', 'td_sf', 'posterior', 'lh_sum', 'lh_sf')
# what schedule_info() has to say of each forest under SMALL: (two-level nodes, stacked nodes); None: some of each
UNITS = dict(chained=(16, 5), ragged=None, fat=(0, 1))

_runs = {}


def run(name, tier, k, schedule):
    """One marginal pass of the case's six columns on a fresh context: dict(info, sweep, counts, lnl [C], and per NAMES the
    full downloads [C, ...]).  Kept per process: the tests of a case share its runs."""
    key = (name, tier, k, schedule)
    if key not in _runs:
        b = cases.build(name, tier, k)
        with hip.Engine(b['flat'], cases.N_COLUMNS, k, tune=SCHEDULES[schedule], keep_td=True) as eng:
            eng.set_masks(b['masks'])
            eng.set_models(b['models'])
            lnl, counts = bu_chain.counted(eng, lambda: eng.marginal_pass(posterior=False, lh=False)[0])
            out = dict(info=eng.schedule_info(), sweep=eng.sweep_schedule(), counts=counts, lnl=np.array(lnl))
            for what, label in zip(TABLES, NAMES):
                out[label] = np.stack([eng.download(what, c) for c in range(cases.N_COLUMNS)])
        _runs[key] = out
    return _runs[key]


def runs(name, tier, k):
    """The four runs of a case, with what says that each took the schedule it is named for."""
    out = {s: run(name, tier, k, s) for s in SCHEDULES}
    _assert_ran(name, out)
    return out


def _assert_ran(name, r):
    """With units: schedule_info() reports the level schedule with two-level and stacked units (chained: 16 and 5; fat: no
    two-level unit and one stacked node, see tests/f81_band_cases.py) and sweep_schedule() the two-level schedule; where there
    are two-level units their brackets are used once each.  On the chained forest each chain takes one launch out of its sweep's
    bracket and nothing else moves (test_gpu_bu_chain.chained, test_gpu_td_chain.chained), elsewhere the switches change no
    count.  The default schedule of so small a forest is the single-launch kernel or the subtree blocks."""
    on, bu_off, td_off = (r[s]['counts'] for s in ('units', 'no_bu_chain', 'no_td_chain'))
    for s in ('units', 'no_bu_chain', 'no_td_chain'):
        scheduled, n_two, n_stacked = r[s]['info']
        assert scheduled and n_stacked > 0 and (n_two > 0) == (name != 'fat'), (name, s, r[s]['info'])
        assert UNITS[name] is None or (n_two, n_stacked) == UNITS[name], (name, s, r[s]['info'])
        assert r[s]['sweep'][0] == hip.SCHEDULE_TWO_LEVEL, (name, s, r[s]['sweep'])
    if name == 'chained':
        assert bu_chain.chained(on, bu_off), (on, bu_off)
        assert td_chain.chained(on, td_off), (on, td_off)
    else:
        assert on == bu_off == td_off, (on, bu_off, td_off)
        assert name == 'fat' or on[3] == on[4] == 1, on
    assert r['default']['sweep'][0] in (hip.SCHEDULE_SINGLE_LAUNCH, hip.SCHEDULE_BLOCKS), r['default']['sweep']


@pytest.mark.parametrize('name, tier, k', cases.CASES, ids=cases.IDS)
def test_against_exact_arithmetic(name, tier, k):
    """Every column under every schedule at the suite's tolerances (the docstring of this file); the worst ratios are printed
    before they are held."""
    flat = cases.build(name, tier, k)['flat']
    r = runs(name, tier, k)
    worst = {}
    for s in SCHEDULES:
        worst[s] = {}
        for c in range(cases.N_COLUMNS):
            e = cases.errors({q: r[s][q][c] for q in ('lnl',) + NAMES}, cases.exact_pass(name, tier, k, c), flat)
            for q in e:
                worst[s][q] = max(worst[s].get(q, 0.0), e[q])
        print('f81-band | {:8s} {:8s} k={:2d} | {:11s} | units {} launches {} | '.format(
            name, tier, k, s, r[s]['info'][1:], r[s]['counts'] + [r[s]['sweep'][0]]) +
            ' '.join('{} {:.3g}'.format(q, worst[s][q]) for q in sorted(worst[s])))
    for s in SCHEDULES:
        assert max(worst[s].values()) < 1, (s, worst[s])


@pytest.mark.parametrize('name, tier, k', cases.CASES, ids=cases.IDS)
def test_rescaling_fired_where_it_must(name, tier, k):
    """A vector whose exact largest entry is below 2^-200 cannot be stored with exponent 0 and inside the band: BU_SF != 0 at
    every such internal node, TD_SF != 0 at every such non-root node.  The host file holds the tiers to where such nodes are:
    the two-level nodes of the bounds tier, the pair units' nodes of the pair and cherry tiers."""
    b = cases.build(name, tier, k)
    flat, h = b['flat'], b['heights']
    r = runs(name, tier, k)
    height = dict(bounds=3, pair=2, cherry=2, straddle=2)[tier]
    for c in range(cases.N_COLUMNS):
        want = cases.exact_pass(name, tier, k, c)
        low_bu = ~flat.is_tip & (want['max_log2'] < -cases.LOG2_BAND)
        low_td = (flat.parent >= 0) & (want['td_log10'].max(axis=1) * LOG2_10 < -cases.LOG2_BAND)
        assert (low_bu & (h == height)).any() and low_td[flat.is_tip].any()
        for s in SCHEDULES:
            assert (r[s]['bu_sf'][c][low_bu] != 0).all(), (s, c, np.flatnonzero(low_bu & (r[s]['bu_sf'][c] == 0)))
            assert (r[s]['td_sf'][c][low_td] != 0).all(), (s, c, np.flatnonzero(low_td & (r[s]['td_sf'][c] == 0)))


@pytest.mark.parametrize('name, tier, k', cases.CASES, ids=cases.IDS)
def test_stored_vectors_keep_the_band_rule(name, tier, k):
    """Needs no reference: every internal node's stored bottom-up vector has its non-zero entries in [2^-200, 2^200] or its
    maximum in [1, 2), under every schedule.  A shortcut that skips a rescale which was due leaves an entry below 2^-200 next
    to a maximum below 1."""
    flat = cases.build(name, tier, k)['flat']
    inner = ~flat.is_tip
    r = runs(name, tier, k)
    for s in SCHEDULES:
        v = r[s]['bu'][:, inner]
        assert np.isfinite(v).all() and (v >= 0).all()
        top = v.max(axis=2)
        low = np.where(v > 0, v, np.inf).min(axis=2)
        in_band = (low >= 2.0 ** -200) & (top <= 2.0 ** 200)
        rescaled = (top >= 1) & (top < 2)
        bad = ~(in_band | rescaled)
        assert not bad.any(), (s, [(int(c), int(np.flatnonzero(inner)[n]), low[c, n], top[c, n]) for c, n in np.argwhere(bad)[:8]])


@pytest.mark.parametrize('name, tier, k', cases.CASES, ids=cases.IDS)
def test_chains_on_and_off_agree_bit_for_bit(name, tier, k):
    """ln L, vectors, exponents, posteriors, sums and their exponents with and without each chain, as 64-bit words, where the
    exponents handed through LDS are not all zero (on the chained forest the launch counts say that the chains ran)."""
    r = runs(name, tier, k)
    on = [r['units'][q] for q in ('lnl',) + NAMES]
    if name == 'chained':
        h = cases.build(name, tier, k)['heights']
        assert (r['units']['bu_sf'][:, h == 3] != 0).any(), 'every exponent into the bottom-up chain is zero'
        assert (r['units']['td_sf'][:, h == 3] != 0).any(), 'every exponent into the top-down chain is zero'
    for off in ('no_bu_chain', 'no_td_chain'):
        assert td_chain.same_bits(on, [r[off][q] for q in ('lnl',) + NAMES]), off


JOINT = [c for c in cases.CASES if c[1] in ('bounds', 'pair')]


@pytest.mark.parametrize('name, tier, k', JOINT, ids=['{}-{}-{}'.format(*c) for c in JOINT])
def test_joint_sweep(name, tier, k):
    """bottom_up(False) with units and on the library's own schedule: ln L against the exact max-product value at LNL_RTOL;
    every arg-max entry that is not the exact first maximum is itself a maximum to 1e-12 (choice_is_a_maximum); where no entry
    differs, the back-traced states are those of the exact tables."""
    b = cases.build(name, tier, k)
    flat = b['flat']
    wants = [cases.joint_exact(name, tier, k, c) for c in range(cases.N_COLUMNS)]
    below = np.flatnonzero(flat.parent >= 0)
    for s in ('units', 'default'):
        with hip.Engine(flat, cases.N_COLUMNS, k, tune=SCHEDULES[s]) as eng:
            eng.set_masks(b['masks'])
            eng.set_models(b['models'])
            lnl = eng.bottom_up(False)
            tables = [eng.download(hip.BUF_JOINT_TABLE, c) for c in range(cases.N_COLUMNS)]
            states = eng.joint_backtrace()
        worst = 0.0
        for c, want in enumerate(wants):
            assert want['loglik'].is_finite()
            worst = max(worst, abs(float((exact.Decimal(float(lnl[c])) - want['loglik']) / want['loglik'])) / LNL_RTOL)
            differs = np.argwhere(tables[c][below] != want['first_maximum'][below])
            for row, i in differs:
                n = int(below[row])
                assert exact.choice_is_a_maximum(want['products'], n, int(i), int(tables[c][n, i])), (s, c, n, int(i))
            if not len(differs):
                expect = np.zeros(flat.n_nodes, dtype=np.int64)
                for n in range(flat.n_nodes):   # parents first
                    p = int(flat.parent[n])
                    expect[n] = want['root_first_maximum'][list(flat.roots).index(n)] if p < 0 else want['first_maximum'][n, expect[p]]
                assert np.array_equal(states[c], expect), (s, c)
        print('f81-band | {:8s} {:8s} k={:2d} | {:11s} | joint lnl {:.3g}'.format(name, tier, k, s, worst))
        assert worst < 1, (s, worst)


CONSUMERS = [c for c in cases.CASES if c[0] == 'chained' and c[1] == 'bounds']


@pytest.mark.parametrize('name, tier, k', CONSUMERS, ids=['{}-{}-{}'.format(*c) for c in CONSUMERS])
def test_consumers_read_the_rescaled_pass(name, tier, k, monkeypatch):
    """loglik_gradient (every column) and expected_history (the columns of cases.CONSUMER_COLUMNS) after a pass with units and
    both chains, each on a fresh context, against loglik_gradient_ref and expected_history_ref by the checkers and at the
    tolerances of their own GPU tests; tests/test_f81_band_cases_host.py holds float64 restatements to the same."""
    monkeypatch.setattr(href, 'history', units.history)   # (the checker's reference and the ratio below: computed once)
    b = cases.build(name, tier, k)
    flat = b['flat']
    worst = dict(gradient=0.0, history=0.0)
    for consumer in worst:
        with hip.Engine(flat, cases.N_COLUMNS, k, tune=SMALL) as eng:
            eng.set_masks(b['masks'])
            eng.set_models(b['models'])
            assert np.isfinite(eng.marginal_pass(posterior=False, lh=False)[0]).all()
            got = eng.loglik_gradient() if consumer == 'gradient' else eng.expected_history(jumps=True, branch_jumps=True)
            post = None if consumer == 'gradient' else np.stack([eng.download(hip.BUF_POSTERIOR, c) for c in range(cases.N_COLUMNS)])
        for c in range(cases.N_COLUMNS) if consumer == 'gradient' else cases.CONSUMER_COLUMNS:
            label = '{} {} k={} column {}'.format(name, tier, k, c)
            column = tuple(x[c] for x in got)
            spec, rates = b['models'][c]
            if consumer == 'gradient':
                ratio = tgradient._ratios(column, flat, b['masks'][c], b['models'][c], label).max()
                worst[consumer] = max(worst[consumer], ratio / tgradient.TOLERANCE)
                assert ratio <= tgradient.TOLERANCE, (label, ratio)
            else:
                h = units.history(flat, b['masks'][c], spec['pi'], *rates, jump_rows=None)
                ratio = max(href.relative_errors(column[0], h['times']).max(), href.relative_errors(column[2], h['branch_jumps']).max(),
                            max(href.relative_errors(column[1][i], h['jumps'][i]).max() for i in range(k)))
                worst[consumer] = max(worst[consumer], ratio / thistory.TOLERANCE)
                thistory._check(column, flat, b['masks'][c], b['models'][c], label, rows=None)
                thistory._check_identities(column, post[c], flat, b['models'][c], label)
    print('f81-band | {:8s} {:8s} k={:2d} | consumers   | gradient {:.3g} history {:.3g}'.format(name, tier, k, worst['gradient'],
                                                                                          worst['history']))
