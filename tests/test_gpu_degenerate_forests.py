"""
GPU tests (``-m gpu``) of the sweeps on forests with nodes of one child, trees of a single tip and stars -- the forests of
tests/degenerate_forest_cases.py (shapes, crowd, grafted), which no draw of FlatForest.random reaches -- against exact arithmetic
(tests/f81_exact_ref.py, tests/matrix_exact_ref.py).  tests/test_degenerate_forest_cases_host.py holds every case to a finite exact
ln L, to the census of what its forest contains and the oracle to the tolerances used here, so nothing is filtered or skipped.

What the cases reach:
    pml_schedule.cpp       pml_check_tree (31-32: only n_children < 0 is refused); kinds_and_heights (87-109: a non-root unary node
                           over a tip is a cherry of one tip, a unary root a stored node); packed_word (112-133: a one-tip cherry
                           has code 1 + 1 = 2, the code of a cherry of more than four tips, told apart by bit 4 only; 14, 15, 16
                           and 17 children around nc < 15 ? nc : 15); two_level_root (196-202) right below and beside a unary
                           node; narrow_levels (897-917) on levels of 500 units next to the roots
    pml_kernels_f81.h      unit_child (486-511: "every cherry among the first four children has 1 - 4 tips", so code - 1 is the
                           number) and f81_gather_issue (537-559: has_t = ... q < code - 1) with one tip; unit_is_fast (513-521) and
                           Gather<G> at G / 4 children and beyond; column_loglik (3440) with its tip branch, over 501 roots
    pml_kernels_misc.h     td_roots_kernel (38-85): the tip branch (a root without children), more than one workgroup of roots
                           and, with the grid capped at eight workgroups, eight passes of its loop over them
and, top-down, the vector of an only child, P (TD_p o BU_p / msg) with nothing else in the product, in the fused, two-level,
stacked, subtree-block and thin-end kernels of the F81 family, the two-GEMM and fused matrix-core sweeps and the sweeps on P(t)
of the eigen models, and HKY.

Per case and schedule, on a fresh context that keeps its top-down vectors (run_case):
    marginal pass   ln L, the bottom-up and top-down vectors as true log10 with equal zero patterns, the posteriors with equal
                    zeros, every node's likelihood sum (roots and lone tips included), both columns, against the exact pass by
                    the checkers of the sibling files (cases.marginal_ratios); bottom_up(True) again: the same bits
    joint sweep     bottom_up(False), the tables and joint_backtrace() against the exact joint pass (cases.joint_ratios)
    selection       select_states MAP, MPPA and MPPA with force_joint against ml.select_map / ml.select_mppa on the device's own
                    posteriors; the selection then serves as masks: a restricted bottom_up(True) is finite
    what ran        schedule_info(), sweep_schedule() and the branches and launches of the plan the library prints under its DEBUG
                    switch, against what the planner takes for the case (expected, assert_ran)
Tolerances: the suite's constants, imported -- LNL_RTOL, POST_RTOL, LOG10_ATOL (LOG10_ATOL_ONE_MATRIX for 65 - 128 states of the
eigen models), f81_exact_ref.tolerance for the F81 family; the likelihood sums of trees without information: see the cases module.
Every case prints its worst error / tolerance on one line ('degenerate | ...', pytest -s); profiles/degenerate_forests_exact.txt
holds those lines from an MI355X.

The random section (test_random_case) holds 24 draws of the fuzz's kinds, state counts, columns and masks on spliced forests with
lone tips appended to the oracle, by the fuzz's own test body, its zero-likelihood contract included.
"""
import numpy as np
import pytest

import degenerate_forest_cases as cases
import test_gpu_fuzz as fuzz
from pastml_amd import hip, ml
from test_gpu_eigen_shapes import FAMILY, OP, PLAN_LINE, _enum, same_bits
from test_gpu_f81_band import SMALL
from test_gpu_parity import log_true

pytestmark = pytest.mark.gpu

BRANCH = {v: name for name, v in _enum('PmlBranch').items()}
OPS = {v: name for name, v in OP.items()}
EIGEN_OPS = ('OP_EIG_TIPS', 'OP_EIG_LEVEL', 'OP_EIG_NARROW', 'OP_EIG_TIER')
FAMILIES = {v: name for name, v in FAMILY.items()}


def thin_ends(k):
    """The scaled-down thin ends of test_thin_ends_as_subtree_blocks_have_the_bits_of_the_level_launches (its `base`)."""
    return dict(BLOCK_NODES=0, SMALL_MAX_NODES=0, SMALL_MANY_NODES=0, THIN_UNITS=400, THIN_BLOCK_NODES=24, NARROW_UNITS=8,
                NO_SUPER=1 if k > 16 else None)


def tune_of(kind, k, schedule):
    """default: the library's own choice; units: the level schedule with two-level and stacked units; blocks: subtree blocks;
    thin: the thin ends as that test scales them down for forests of thousands of tips -- no level here holds more than 400
    units, so the planner declines --; thinner: the same with thin levels of at most 32 units and bins of 8, which these forests
    have; other: the eigen models without the two-GEMM sweeps and without the vector-unit joint sweep; levels: the two-GEMM sweeps
    with a launch per level where the library would cut tiers of subtree blocks; capped: eight workgroups per launch, so that
    td_roots_kernel's grid (4 waves of 64 / G roots per workgroup: 64 roots a pass at 64 states) walks the 501 roots of `crowd` in
    eight passes -- uncapped, the grid covers every root in one."""
    return {'default': None, 'units': SMALL, 'blocks': dict(SMALL_MAX_NODES=0, BLOCK_NODES=32), 'thin': thin_ends(k),
            'thinner': dict(thin_ends(k), THIN_UNITS=32, THIN_BLOCK_NODES=8),
            'other': dict(NO_EIGEN_GEMM=1, NO_EIGEN_JOINT_VALU=1), 'levels': dict(NO_EIGG_TIERS=1),
            'capped': dict(GRID_CAP=8)}[schedule]


def schedules_of(kind, k, name):
    if kind == 'F81':
        return ('default', 'units', 'blocks') + (('thin', 'thinner') if name != 'shapes' else ())
    if kind == 'EIGEN':
        return ('default', 'other') + (('levels',) if name != 'shapes' else ()) + (('capped',) if name == 'crowd' else ())
    return ('default',)


RUNS = [(kind, k, name, s) for kind, k, name in cases.CASES for s in schedules_of(kind, k, name)]


def read_plan(text):
    """dict(branches: the set of their names, ops: name -> the largest count of a launch of it, families: the set of the eigen
    launches' families) of the launches the library listed."""
    rows = [tuple(int(x) for x in m.groups()) for m in PLAN_LINE.finditer(text)]
    assert rows, 'the library printed no launch plan'
    ops = {}
    for r in rows:
        ops[OPS[r[1]]] = max(ops.get(OPS[r[1]], 0), r[5])
    return dict(branches={BRANCH[r[0]] for r in rows}, ops=ops, families={FAMILIES[r[3]] for r in rows if OPS[r[1]] in EIGEN_OPS})


def run_case(kind, k, name, schedule, capfd):
    """Everything one context computes for a case: dict(columns [2] in the terms of cases.marginal_ratios, joint [2] in those of
    cases.joint_ratios, info, sweep, plans (bottom-up, top-down, joint))."""
    b = cases.build(kind, k, name)
    flat, masks, C = b['flat'], b['masks'], 2
    with hip.Engine(flat, C, k, tune=dict(tune_of(kind, k, schedule) or {}, DEBUG=1), keep_td=True) as eng:
        eng.set_models(list(zip(b['specs'], b['rates'])))
        eng.set_masks(masks)
        out = dict(info=eng.schedule_info(), sweep=eng.sweep_schedule())
        capfd.readouterr()
        lnl = np.array(eng.bottom_up(True))
        plans = [read_plan(capfd.readouterr().err)]
        post, lh_sum, lh_sf = eng.top_down_marginals()
        plans.append(read_plan(capfd.readouterr().err))
        out['columns'] = [dict(lnl=float(lnl[c]), bu=eng.download(hip.BUF_BU, c), bu_sf=eng.download(hip.BUF_BU_SF, c),
                               td=eng.download(hip.BUF_TD, c), td_sf=eng.download(hip.BUF_TD_SF, c), posterior=post[c],
                               lh_sum=lh_sum[c], lh_sf=lh_sf[c]) for c in range(C)]
        assert same_bits(lnl, eng.bottom_up(True)), 'bottom_up(True) after the pass gives other bits'
        capfd.readouterr()
        lnl_j = np.array(eng.bottom_up(False))
        plans.append(read_plan(capfd.readouterr().err))
        out['joint'] = [dict(loglik=float(lnl_j[c]), table=eng.download(hip.BUF_JOINT_TABLE, c),
                             bu_log10=log_true(eng.download(hip.BUF_BU, c), eng.download(hip.BUF_BU_SF, c))) for c in range(C)]
        states = eng.joint_backtrace()
        for c in range(C):
            out['joint'][c]['states'] = states[c]
        # MAP / MPPA on the device against the host restatement, on the device's own posteriors (as tests/test_gpu_fuzz.py)
        assert np.all(np.isfinite(post))
        for method, fj in (('MPPA', True), ('MPPA', False), ('MAP', False)):
            eng.set_masks(masks)
            eng.bottom_up(True)
            eng.top_down_marginals(posterior=False, lh=False)
            sel, nsel = eng.select_states(method, force_joint=fj)
            for c in range(C):
                if method == 'MAP':
                    ref_sel, ref_k = ml.select_map(post[c]), np.ones(flat.n_nodes, dtype=int)
                else:
                    ref_sel, ref_k = ml.select_mppa(post[c], states[c].astype(np.int64) if fj else None)
                assert np.array_equal(nsel[c], ref_k), (method, fj, c)
                assert np.array_equal(sel[c], ref_sel), (method, fj, c)
            assert np.all(np.isfinite(eng.bottom_up(True))), (method, fj, 'the selection as masks')
        capfd.readouterr()
    out['plans'] = plans
    return out


LEVELS = ('BU_FUSED', 'TD_LEVELS')        # the F81 family's level schedule without units
PLAIN = ('BU_PLAIN', 'TD_LEVELS')         # sweeps on P(t): per-branch pass and plain level launches


def expected(kind, k, name, schedule, census):
    """(branch of the marginal bottom-up sweep, of the top-down sweep, of the joint sweep) that pml_plan_bottom_up /
    pml_plan_top_down take for a case -- the schedule a run is named for where the forest admits it, and what the planner chooses
    instead where it declines:
        F81     beyond 256 states there are no multi-level kernels: the level schedule whatever the switches.  Two-level units
                need lane groups of 8 (16 < k <= 64) and a two-level root; `crowd` has none.  The joint sweep is fused with the
                cherries while the masks are one word.
        EIGEN   the two-GEMM sweeps up to 128 states, in tiers of subtree blocks on the forests with thin levels (crowd, grafted)
                unless switched to levels; the vector-unit joint sweep up to 64 states; without them the fused matrix-core
                sweeps at 16 and 20 states (KS 4 and 5) and P(t) in HBM elsewhere.
        HKY     P(t) in registers: plain level launches without the per-branch pass."""
    if kind == 'F81':
        joint = 'BU_FUSED_JOINT' if k <= 64 else 'BU_PLAIN'
        if k > 256:
            return LEVELS + (joint,)
        if schedule == 'default':
            return ('BU_ONE_LAUNCH', 'TD_ONE_LAUNCH', joint)
        if schedule == 'blocks':
            return ('BU_BLOCKS', 'TD_BLOCKS', joint)
        if schedule == 'units' and 16 < k <= 64 and census['two_level_roots'] > 0:
            return ('BU_SUPER', 'TD_SUPER', joint)
        if schedule == 'thinner':
            return THINNER[name] + (joint,)
        return LEVELS + (joint,)
    if kind == 'HKY':
        return PLAIN + ('BU_PLAIN',)
    if schedule == 'other' or k > 128:
        return ('BU_EIG_FUSED', 'TD_EIG_FUSED', 'BU_EIG_FUSED') if k in (16, 20) and schedule == 'other' else PLAIN + ('BU_PLAIN',)
    tiers = name != 'shapes'
    return ('BU_GEMM_TIERS' if tiers and schedule != 'levels' else 'BU_GEMM', 'TD_GEMM',
            'BU_PLAIN' if k > 64 else 'BU_EIGJ_TIERS' if tiers else 'BU_EIGJ')


# what the planner makes of THIN_UNITS = 32 (pml_plan_thin_ends): tiers of subtree blocks bottom-up, bins of subtrees top-down
# (on `crowd` the thin levels of the 40-tip tree end in levels of one unit, which leaves fewer than three for a tier: the
# bottom-up sweep keeps a launch per level)
THINNER = dict(crowd=('BU_FUSED', 'TD_DEEP'), grafted=('BU_THIN', 'TD_DEEP'))


def assert_ran(kind, k, name, schedule, r):
    bu, td, joint = r['plans']
    census = cases.census(cases.forest_of(kind, name))
    want = expected(kind, k, name, schedule, census)
    assert (bu['branches'], td['branches'], joint['branches']) == ({want[0]}, {want[1]}, {want[2]}), (want, r['plans'])
    scheduled, n_two, n_stacked = r['info']
    if want[0] == 'BU_SUPER':
        assert scheduled and n_two == census['two_level_roots'] and r['sweep'][0] == hip.SCHEDULE_TWO_LEVEL, (r['info'], r['sweep'])
        assert 'OP_SUPER' in bu['ops'] and 'OP_SUPER' in td['ops'], (bu, td)
    elif kind == 'F81':
        assert not scheduled and r['sweep'][0] == dict(BU_ONE_LAUNCH=hip.SCHEDULE_SINGLE_LAUNCH, BU_BLOCKS=hip.SCHEDULE_BLOCKS).get(
            want[0], hip.SCHEDULE_LEVELS), (r['info'], r['sweep'])
        assert (r['sweep'][1] > 0) == (want[0] == 'BU_BLOCKS') and ('OP_BLOCKS' in bu['ops']) == (want[0] in ('BU_BLOCKS', 'BU_THIN'))
    else:
        assert r['sweep'][0] == hip.SCHEDULE_OTHER_MODEL
        assert bu['families'] == ({'EIG_GEMM'} if 'GEMM' in want[0] else {'EIG_FUSED'} if 'EIG_FUSED' in want[0] else set())
        assert joint['families'] == ({'EIG_JOINT'} if 'EIGJ' in want[2] else {'EIG_FUSED'} if 'EIG_FUSED' in want[2] else set())
        assert ('OP_PREP' in bu['ops']) == (want[0] == 'BU_PLAIN' and kind == 'EIGEN')
    if name == 'crowd':
        # a level of some 500 nodes next to the roots is above every narrow limit: it has a launch of its own
        widest = cases.NARROW_GEMM
        if want[0] == 'BU_GEMM':
            assert bu['ops']['OP_EIG_LEVEL'] > widest, bu
        if want[1] == 'TD_GEMM':
            assert td['ops']['OP_EIG_LEVEL'] > widest, td
        if want[:2] in (LEVELS, PLAIN):
            assert bu['ops']['OP_LEVEL'] > 256 and td['ops']['OP_LEVEL'] > 256, (bu, td)


@pytest.mark.parametrize('kind, k, name, schedule', RUNS, ids=['{}{}-{}-{}'.format(*r) for r in RUNS])
def test_against_exact_arithmetic(kind, k, name, schedule, capfd):
    """One context per case and schedule (the docstring of this file): both columns of the marginal pass and of the joint sweep at
    the suite's tolerances, the selection, and what ran.  The worst ratios are printed before they are held."""
    b = cases.build(kind, k, name)
    flat = b['flat']
    wants = [cases.exact_pass(kind, k, name, c) for c in range(2)]
    joints = [cases.joint_exact(kind, k, name, c) for c in range(2)]
    for want, joint in zip(wants, joints):   # (on the exact side, before the engine opens)
        assert want['loglik'].is_finite() and joint['loglik'].is_finite()
        if kind != 'F81':
            assert want['min_message_ratio'] > cases.eigen_cases.MIN_MESSAGE_RATIO
            assert joint['min_best_ratio'] > cases.eigen_cases.MIN_MESSAGE_RATIO
    r = run_case(kind, k, name, schedule, capfd)
    worst = {}
    failure = None
    for c in range(2):
        try:
            ratios = cases.marginal_ratios(kind, k, r['columns'][c], wants[c], flat)
            ratios.update({'joint_' + q: v for q, v in cases.joint_ratios(
                kind, k, r['joint'][c], joints[c], flat, b['masks'][c], b['specs'][c], b['rates'][c]).items()})
        except AssertionError as e:   # (a difference in kind -- zero patterns, a table entry: reported after the line is printed)
            failure = failure or (c, e)
            continue
        for q, v in ratios.items():
            worst[q] = max(worst.get(q, 0.0), v)
    bu, td, joint = (' '.join(sorted(p['branches'])) for p in r['plans'])
    print('degenerate | {:5s} k={:3d} {:7s} | {:7s} | units {} sweep {} | {} / {} / {} | '.format(
        kind, k, name, schedule, r['info'], r['sweep'], bu, td, joint)
        + ' '.join('{} {:.3g}'.format(q, worst[q]) for q in sorted(worst)))
    assert failure is None, failure
    assert_ran(kind, k, name, schedule, r)
    assert max(worst.values()) < 1, worst


@pytest.mark.parametrize('seed', range(cases.RANDOM_SEEDS))
def test_random_case(seed, monkeypatch):
    """tests/test_gpu_fuzz.py's test body -- ln L, bottom-up vectors, posteriors, totals, the joint sweep, the selection, and a zero
    likelihood raised on both sides with the same pair of nodes -- on the draws of cases.draw_random_case.  The host file asserts
    that the reference has an answer for every seed, so nothing is skipped."""
    monkeypatch.setattr(fuzz, 'draw_case', cases.draw_random_case)
    try:
        fuzz.test_random_case(seed)
    except pytest.skip.Exception as e:
        pytest.fail('seed {}: {}'.format(seed, e))
