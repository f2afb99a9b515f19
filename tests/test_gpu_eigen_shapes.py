"""
GPU tests (``-m gpu``) of the sum sweeps of the matrix models against exact arithmetic (tests/matrix_exact_ref.py, 50-digit
decimal on the doubles the device is handed), at every lane shape of the two-GEMM sweeps (pml_kernels_eigen_gemm.h): every state
count from 2 to 64 -- top-down KS = ceil(k / 4) from 1 to 16, bottom-up and tips KS rounded up to even; odd KS with states 4s + hi,
even KS in pairs; operands in registers below KS 5, in LDS above, one transposed matrix in LDS above KS 16; 0 to 7 states of padding
--, each in its level form and in its several-levels-per-launch ("narrow") form, and the one-matrix form of 65 - 128 states at its
shape boundaries.  The inputs are those of tests/eigen_shape_cases.py (forests S and L, a column of observed tips next to a column of
masks of every kind); tests/test_matrix_exact_ref.py holds the oracle to the same tolerances on the same inputs.

Each case asserts which kernels ran, from the launch plan the library prints under its DEBUG switch (one line per launch:
pml_api.hip, run_plan), and the deep cases assert that rescaling fired (BUF_BU_SF, BUF_TD_SF).

Tolerances: the suite's constants -- ln L LNL_RTOL, vectors LOG10_ATOL in log10 (1e-9 for the one-matrix form, as in
test_eigen_sum_sweeps_of_65_to_128_states), posteriors POST_RTOL with atol 1e-300, the nodes' likelihood sums LNL_RTOL on their log10
-- and, since 8 x the worst error measured on an MI355X (profiles/eigen_shapes_exact.txt) is below every one of them, that instead:
see TOLERANCES.
Every case prints its worst errors and their ratio to the tolerance (pytest -s).
"""
import os
import re

import numpy as np
import pytest

import eigen_shape_cases as cases
import matrix_exact_ref as exact
from pastml_amd import hip
from test_gpu_parity import LNL_RTOL, LOG10_ATOL, POST_RTOL, log_true

pytestmark = pytest.mark.gpu

# Tolerance per group of kernels and quantity: 'gemm' the two-GEMM form up to 64 states, 'sym' its one-matrix form of 65 - 128
# states, 'other' the fused matrix-core sweeps, the sweeps on materialised P(t) and HKY.  SUITE: the suite's constants.  MEASURED:
# the worst error of the group's cases in one run on an MI355X, the lines "worst" of profiles/eigen_shapes_exact.txt (relative
# error of ln L; largest difference of a log10 vector entry; relative error of a posterior; relative error of the log10 of a
# node's likelihood sum).  Every 8 x MEASURED is below its constant, so that is what the tests carry: the device is 7 to 1e5 times
# closer to exact arithmetic than the suite's constants ask, and a kernel that loses one of those digits is a change to look at.
SUITE = dict(gemm=dict(lnl=LNL_RTOL, log10=LOG10_ATOL, post=POST_RTOL, lh=LNL_RTOL),
             sym=dict(lnl=LNL_RTOL, log10=cases.LOG10_ATOL_ONE_MATRIX, post=POST_RTOL, lh=LNL_RTOL),
             other=dict(lnl=LNL_RTOL, log10=LOG10_ATOL, post=POST_RTOL, lh=LNL_RTOL))
MEASURED = dict(gemm=dict(lnl=6.21e-15, log10=1.35e-11, post=3.05e-11, lh=1.34e-14),
                sym=dict(lnl=8.27e-15, log10=2.53e-11, post=5.83e-11, lh=2.22e-14),
                other=dict(lnl=1.04e-16, log10=1.14e-13, post=1.78e-13, lh=2.22e-16))
TOLERANCES = {g: {q: min(SUITE[g][q], 8 * MEASURED[g][q]) for q in SUITE[g]} for g in SUITE}


def _enum(name):
    """The enumerators of ``enum name`` in pml_schedule.h, name -> value (the plan lines print these numbers)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pastml_amd', 'csrc', 'pml_schedule.h')
    with open(path) as f:
        text = f.read()
    body = re.search(r'enum ' + name + r' \{(.*?)\};', text, re.S).group(1)
    body = re.sub(r'//[^\n]*', '', body)
    return {word.strip(): i for i, word in enumerate(w for w in body.split(',') if w.strip())}


OP, FAMILY = _enum('PmlOp'), _enum('PmlEigenFamily')
PLAN_LINE = re.compile(r'pml plan: branch (\d+) op (\d+) list (\d+) kind (\d+) first (-?\d+) count (-?\d+) ')


def read_plan(text):
    """[(op, kind, count)] of the launches the library listed, in order."""
    return [(int(m.group(2)), int(m.group(4)), int(m.group(6))) for m in PLAN_LINE.finditer(text)]


def has(plan, op, family=None, min_count=1):
    return any(o == OP[op] and (family is None or kind == FAMILY[family]) and count >= min_count for o, kind, count in plan)


def eigen_families(plan):
    """The kernel families of the plan's eigen launches."""
    eig = (OP['OP_EIG_TIPS'], OP['OP_EIG_LEVEL'], OP['OP_EIG_NARROW'], OP['OP_EIG_TIER'])
    return {kind for o, kind, _ in plan if o in eig}


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def run_marginal(flat, k, specs, rates, masks, capfd, tune=None):
    """One marginal pass of C columns.  Returns ([per column: the results in the terms of the exact pass plus bu_sf, td_sf], the
    bottom-up sweep's plan, the top-down sweep's plan)."""
    C = len(specs)
    with hip.Engine(flat, C, k, tune=dict(tune or {}, DEBUG=1), keep_td=True) as eng:
        eng.set_models(list(zip(specs, rates)))
        eng.set_masks(np.asarray(masks))
        capfd.readouterr()
        lnl = eng.bottom_up(True)
        bu_plan = read_plan(capfd.readouterr().err)
        post, lh_sum, lh_sf = eng.top_down_marginals()
        td_plan = read_plan(capfd.readouterr().err)
        out = []
        for c in range(C):
            bu, bu_sf = eng.download(hip.BUF_BU, c), eng.download(hip.BUF_BU_SF, c)
            td, td_sf = eng.download(hip.BUF_TD, c), eng.download(hip.BUF_TD_SF, c)
            out.append(dict(loglik=float(lnl[c]), bu_log10=log_true(bu, bu_sf), td_log10=log_true(td, td_sf), posterior=post[c],
                            lh_log10=np.log10(lh_sum[c]) - lh_sf[c], bu_sf=bu_sf, td_sf=td_sf))
        again = eng.bottom_up(True)
        assert same_bits(lnl, again), 'bottom_up(True) after the pass gives other bits'
    assert bu_plan and td_plan, 'the library printed no launch plan'
    return out, bu_plan, td_plan


def check(label, k, got, want, group):
    """The device's results of one column against the exact pass; prints the worst errors; returns error / tolerance per quantity."""
    assert want['loglik'].is_finite() and want['min_message_ratio'] > cases.MIN_MESSAGE_RATIO
    err = cases.errors(got, want)
    ratio = {key: err[key] / TOLERANCES[group][key] for key in err}
    print('eigen-shapes {}: {}'.format(label, '  '.join('{} {:.3g} ({:.3g} of tol)'.format(a, err[a], ratio[a]) for a in sorted(err))))
    assert max(ratio.values()) < 1, (label, err, ratio)
    return ratio


def assert_two_gemm_family(plans):
    for plan in plans:
        assert eigen_families(plan) == {FAMILY['EIG_GEMM']}, plan


@pytest.mark.parametrize('which', ['S', 'L'])
@pytest.mark.parametrize('k', cases.STATES_TWO_MATRICES)
def test_every_state_count_of_the_two_gemm_sweeps(k, which, capfd):
    """
    ln L, the bottom-up and top-down vectors as true log10 values with equal zero patterns, the posteriors and the nodes' likelihood
    sums of both columns against the exact pass; bottom_up(True) after the pass returns the same ln L bits.  Forest S runs the tip
    launch and the narrow kernel; forest L must run a level launch and a narrow launch of the two-GEMM family in each sweep (read
    from the plan, not from the forest's level sizes).  Column 0's tips are all one-hot: the gathered first product's precondition.
    (An exact pass over L at 64 states takes 4 s per column, so both columns stay at every k.)
    """
    b = cases.build(k, which)
    flat = b['flat']
    assert np.all(b['masks'][0][flat.is_tip].sum(axis=1) == 1)
    wants = [cases.exact_pass(k, which, c) for c in range(2)]
    assert all(w['loglik'].is_finite() for w in wants)   # (positive likelihood, before the engine is opened)
    got, bu_plan, td_plan = run_marginal(flat, k, b['specs'], b['rates'], b['masks'], capfd)
    assert_two_gemm_family((bu_plan, td_plan))
    assert has(bu_plan, 'OP_EIG_TIPS', 'EIG_GEMM', 0)
    if which == 'L':
        for plan in (bu_plan, td_plan):
            assert has(plan, 'OP_EIG_LEVEL', 'EIG_GEMM', 129), plan
            assert has(plan, 'OP_EIG_NARROW', 'EIG_GEMM', 2), plan
    else:
        assert has(bu_plan, 'OP_EIG_NARROW', 'EIG_GEMM', 2), bu_plan
    for c in range(2):
        check('k={} forest={} column={}'.format(k, which, c), k, got[c], wants[c], 'gemm')


@pytest.mark.parametrize('k', cases.STATES_ONE_MATRIX)
def test_one_matrix_form_at_its_shape_boundaries(k, capfd):
    """65 - 128 states (one matrix in LDS, EigGemm::SYM) at the first and last k of each of its four lane shapes, on forest S, both
    columns, with the comparisons above.  (Its level kernels: test_eigen_sum_sweeps_of_65_to_128_states, against the oracle.)"""
    b = cases.build(k, 'S')
    flat = b['flat']
    assert np.all(b['masks'][0][flat.is_tip].sum(axis=1) == 1)
    wants = [cases.exact_pass(k, 'S', c) for c in range(2)]
    assert all(w['loglik'].is_finite() for w in wants)
    got, bu_plan, td_plan = run_marginal(flat, k, b['specs'], b['rates'], b['masks'], capfd)
    assert_two_gemm_family((bu_plan, td_plan))
    assert has(bu_plan, 'OP_EIG_TIPS', 'EIG_GEMM', 0) and has(bu_plan, 'OP_EIG_NARROW', 'EIG_GEMM', 2), bu_plan
    for c in range(2):
        check('k={} forest=S column={}'.format(k, c), k, got[c], wants[c], 'sym')


def took_two_gemm(bu_plan, td_plan):
    assert_two_gemm_family((bu_plan, td_plan))


def took_fused_matrix_core(bu_plan, td_plan):
    for plan in (bu_plan, td_plan):
        assert eigen_families(plan) == {FAMILY['EIG_FUSED']}, plan


def took_materialised(bu_plan, td_plan):
    """bu_matrix_kernel / td_matrix_kernel on P(t) in HBM: the per-branch pass and plain level launches, no eigen launch."""
    assert has(bu_plan, 'OP_PREP', None, 0) and has(bu_plan, 'OP_LEVEL') and has(td_plan, 'OP_LEVEL')
    assert not eigen_families(bu_plan) and not eigen_families(td_plan)


def took_hky_in_registers(bu_plan, td_plan):
    """Plain level launches WITHOUT the per-branch pass: P(t) is built in registers."""
    assert not has(bu_plan, 'OP_PREP', None, 0) and has(bu_plan, 'OP_LEVEL') and has(td_plan, 'OP_LEVEL')
    assert not eigen_families(bu_plan) and not eigen_families(td_plan)


# (kind, k, tune, the family it must take, tolerance group)
DEEP = [('EIGEN', 11, None, took_two_gemm, 'gemm'),          # odd KS, operands in registers
        ('EIGEN', 16, None, took_two_gemm, 'gemm'),          # even KS, registers
        ('EIGEN', 20, None, took_two_gemm, 'gemm'),          # LDS
        ('EIGEN', 43, None, took_two_gemm, 'gemm'),          # KS 11
        ('EIGEN', 64, None, took_two_gemm, 'gemm'),
        ('EIGEN', 65, None, took_two_gemm, 'sym'),           # one-matrix form
        ('EIGEN', 20, dict(NO_EIGEN_GEMM=1), took_fused_matrix_core, 'other'),   # pml_kernels_eigen_mfma.h
        ('EIGEN', 40, dict(NO_EIGEN_GEMM=1), took_materialised, 'other'),        # pml_kernels_matrix.h on P(t) in HBM
        ('HKY', 4, None, took_hky_in_registers, 'other')]                        # pml_kernels_matrix.h, P(t) in registers


@pytest.mark.parametrize('kind,k,tune,took,group', DEEP, ids=['{}{}{}'.format(d[0], d[1], '-no-gemm' if d[2] else '') for d in DEEP])
def test_rescaling_on_a_deep_caterpillar(kind, k, tune, took, group, capfd):
    """
    One observed tip per level (tip branch 0.8, spine 0.05), as deep as it takes the exact bottom-up vector of the root below
    2^-800: four trips through the rescaling band at least, in node_lazy_rescale of the two-GEMM kernels (per child bottom-up; on
    x = TD_p o BU_p / msg top-down), lazy_rescale<16, NT> of the fused matrix-core sweeps and the three sites of
    pml_kernels_matrix.h.  Each case takes the family it names, agrees with the exact pass, and has non-zero BUF_BU_SF and
    BUF_TD_SF at interior nodes of the spine.
    """
    d = cases.deep_caterpillar(kind, k)
    want = cases.deep_exact(kind, k)
    assert want['loglik'].is_finite()
    assert d['depth'] % 50 == 0 and want['bu_log10'][0].max() * exact.LOG2_OF_10 < cases.DEEP_LOG2
    got, bu_plan, td_plan = run_marginal(d['flat'], k, [d['spec']], [d['rates']], d['masks'][None], capfd, tune)
    took(bu_plan, td_plan)
    check('deep {} k={}{} depth={}'.format(kind, k, ' NO_EIGEN_GEMM' if tune else '', d['depth']), k, got[0], want, group)
    inner = np.array(d['spine'][1:-1])
    assert np.any(got[0]['bu_sf'][inner] != 0), 'no bottom-up rescaling on the spine'
    assert np.any(got[0]['td_sf'][inner] != 0), 'no top-down rescaling on the spine'
    print('eigen-shapes deep {} k={}: {} distinct bottom-up and {} distinct top-down scales on the spine'.format(
        kind, k, len(np.unique(got[0]['bu_sf'][inner])), len(np.unique(got[0]['td_sf'][inner]))))


@pytest.mark.parametrize('k', [5, 20])
def test_rescaling_inside_a_level_launch(k, capfd):
    """140 trees whose root has one child, a polytomy of observed tips in rare states on long branches: the polytomies are one
    level of 140 nodes, above the narrow limit, so a LEVEL launch of the two-GEMM family multiplies their children's messages, and
    the exact vectors of those nodes lie below 2^-200: the product leaves the band inside the loop over the children."""
    d = cases.polytomy_forest(k)
    want = cases.polytomy_exact(k)
    assert want['loglik'].is_finite()
    assert np.all(want['bu_log10'][d['polytomies']].max(axis=1) * exact.LOG2_OF_10 < -200)
    got, bu_plan, td_plan = run_marginal(d['flat'], k, [d['spec']], [d['rates']], d['masks'][None], capfd)
    took_two_gemm(bu_plan, td_plan)
    assert (OP['OP_EIG_LEVEL'], FAMILY['EIG_GEMM'], len(d['polytomies'])) in bu_plan, bu_plan
    assert not has(bu_plan, 'OP_EIG_NARROW') and not has(bu_plan, 'OP_EIG_TIER', None, 0), bu_plan
    check('polytomies k={} fan={}'.format(k, d['fan']), k, got[0], want, 'gemm')
    assert np.all(got[0]['bu_sf'][d['polytomies']] != 0), 'no rescaling on the level of the polytomies'
    tips = d['flat'].is_tip
    assert np.any(got[0]['td_sf'][tips] != 0)


@pytest.mark.parametrize('k', cases.JOINT_STATES)
def test_joint_sweep_at_the_state_counts_of_the_new_shapes(k):
    """bottom_up(False) on forest S, both columns, without the DEBUG switch: ln L against the exact max-product value, and the
    assertions of cases.joint_errors (tables, vectors' zero patterns, the back-traced scenario).  Every state count, the plans, the
    level launches and the other forms of the joint sweep: tests/test_gpu_joint_shapes.py."""
    b = cases.build(k, 'S')
    flat = b['flat']
    wants = [cases.joint_exact(k, 'S', c) for c in range(2)]
    assert all(w['loglik'].is_finite() for w in wants)
    with hip.Engine(flat, 2, k) as eng:
        eng.set_models(list(zip(b['specs'], b['rates'])))
        eng.set_masks(b['masks'])
        lnl = eng.bottom_up(False)
        got = [dict(loglik=float(lnl[c]), table=eng.download(hip.BUF_JOINT_TABLE, c),
                    bu_log10=log_true(eng.download(hip.BUF_BU, c), eng.download(hip.BUF_BU_SF, c))) for c in range(2)]
        states = eng.joint_backtrace()
    for c in range(2):
        err = cases.joint_errors(dict(got[c], states=states[c]), wants[c], flat, b['masks'][c], b['specs'][c], b['rates'][c])
        print('eigen-shapes joint k={} column={}: lnl {:.3g} ({:.3g} of tol)'.format(k, c, err['lnl'], err['lnl'] / LNL_RTOL))
        assert err['lnl'] < LNL_RTOL and err['log10'] < LOG10_ATOL and err['scenario'] < 1, err
