"""
GPU tests (``-m gpu``) of the joint (max-product) sweep of the matrix models against exact arithmetic (tests/matrix_exact_ref.py,
joint_pass and scenario_log_probability: 50-digit decimal on the doubles the device is handed), at every width of the vector-unit
kernels (pml_kernels_eigen_joint.h): every state count from 2 to 64 -- npw = 64 / k node slots per wavefront and 64 - npw k idle tail
lanes; 0 to 3 padding columns; A^-1 transposed with stride 32 up to 32 states and 64 beyond; the column loop unrolled up to 32
states; the level kernel pipelined up to 32 states and the plain loop beyond --, each in the tip launches and the narrow launch
(forest S) and in a level launch of three passes per wave with chunked tip passes (forest J(k)), with rescaling on a spine and inside
a level launch, and the other forms of the joint sweep: HKY with P(t) in registers, the sweeps on materialised P(t), the fused
matrix-core sweep and the path beyond 64 states.  The inputs are those of tests/eigen_shape_cases.py;
tests/test_matrix_exact_ref.py holds the oracle to the same assertions on the same inputs.

Every case runs bottom_up(False), downloads BUF_JOINT_TABLE, BUF_BU and BUF_BU_SF, then joint_backtrace(), and asserts on every column
    the plan      which kernels ran, from the launch plan the library prints under its DEBUG switch (read_plan);
    ln L          against the exact max-product value;
    the vectors   of the internal nodes as true log10 values: equal zero patterns, finite entries in tolerance;
    the tables    every entry of every non-root node is a maximum of the exact products, up to products equal to 1e-12;
    the scenario  the back-traced states are allowed by their masks, and the exact ln probability of the scenario lies within
                  (nodes of the tree) x 1e-12 of the exact maximum: each choice is within 1e-12 relative of its row's best, so the
                  product is within (1 + 1e-12)^n;
and before the engine is opened, on the exact side: a finite likelihood, and no message entry below MIN_MESSAGE_RATIO of its
vector's largest (no clamp of negative P(t) dust can have acted on a maximum; the relative tie test is meaningful in every row).

Tolerances: the suite's constants -- ln L LNL_RTOL, vectors LOG10_ATOL in log10 --, or 8 x the worst error measured on an MI355X
(profiles/joint_shapes_exact.txt) where that is below the constant: see TOLERANCES.  The tie width and the scenario bound are
derived, not measured, and stay.  Every case prints its worst errors and their ratio to the tolerance (pytest -s).
"""
import numpy as np
import pytest

import eigen_shape_cases as cases
import matrix_exact_ref as exact
from pastml_amd import hip
from test_gpu_eigen_shapes import FAMILY, OP, eigen_families, has, read_plan, same_bits
from test_gpu_parity import LNL_RTOL, LOG10_ATOL, log_true

pytestmark = pytest.mark.gpu

# Tolerance per group of kernels and quantity: 'valu32' the vector-unit joint kernels up to 32 states, 'valu64' beyond, 'other' HKY,
# the sweeps on materialised P(t), the fused matrix-core sweep and the path beyond 64 states.  SUITE: the suite's constants.
# MEASURED: the worst error of the group's cases in one run on an MI355X, the lines "worst" of profiles/joint_shapes_exact.txt
# (relative error of ln L; largest difference of a log10 vector entry).  Where 8 x MEASURED is below the constant the tests carry
# that.  'scenario' is in units of its derived bound, (nodes of the tree) x 1e-12, and is not tightened.
SUITE = dict(valu32=dict(lnl=LNL_RTOL, log10=LOG10_ATOL), valu64=dict(lnl=LNL_RTOL, log10=LOG10_ATOL),
             other=dict(lnl=LNL_RTOL, log10=LOG10_ATOL))
MEASURED = dict(valu32=dict(lnl=1.56e-15, log10=1.97e-12),
                valu64=dict(lnl=7.11e-15, log10=3.47e-12),
                other=dict(lnl=9.97e-16, log10=3.78e-13))
TOLERANCES = {g: {q: min(SUITE[g][q], 8 * MEASURED[g][q]) for q in SUITE[g]} for g in SUITE}


def group_of(k):
    return 'valu32' if k <= 32 else 'valu64'


def run_joint(flat, k, specs, rates, masks, capfd, tune=None):
    """One joint sweep and back-trace of C columns.  Returns ([per column: dict(loglik, bu, bu_sf, bu_log10, table, states)], the
    bottom-up sweep's plan)."""
    C = len(specs)
    with hip.Engine(flat, C, k, tune=dict(tune or {}, DEBUG=1)) as eng:
        eng.set_models(list(zip(specs, rates)))
        eng.set_masks(np.asarray(masks))
        printed = capfd.readouterr().out
        lnl = eng.bottom_up(False)
        plan = read_plan(capfd.readouterr().err)
        print(printed, end='')   # (what the test has printed so far stays in its output)
        out = []
        for c in range(C):
            table = eng.download(hip.BUF_JOINT_TABLE, c)
            bu, bu_sf = eng.download(hip.BUF_BU, c), eng.download(hip.BUF_BU_SF, c)
            out.append(dict(loglik=float(lnl[c]), bu=bu, bu_sf=bu_sf, bu_log10=log_true(bu, bu_sf), table=table))
        states = eng.joint_backtrace()
        print(capfd.readouterr().out, end='')   # (without the back-trace's plan)
        for c in range(C):
            out[c]['states'] = states[c]
    assert plan, 'the library printed no launch plan'
    return out, plan


def precondition(want):
    """On the exact side, before the engine opens."""
    assert want['loglik'].is_finite()
    assert want['min_best_ratio'] > cases.MIN_MESSAGE_RATIO, want['min_best_ratio']


def check(label, got, want, flat, masks, spec, rates, group):
    """The device's results of one column against the exact joint pass; prints the worst errors; returns error / tolerance."""
    err = cases.joint_errors(got, want, flat, masks, spec, rates)
    ratio = dict(lnl=err['lnl'] / TOLERANCES[group]['lnl'], log10=err['log10'] / TOLERANCES[group]['log10'], scenario=err['scenario'])
    print('joint-shapes {} [{}]: {}'.format(label, group, '  '.join('{} {:.3g} ({:.3g} of tol)'.format(a, err[a], ratio[a])
                                                                      for a in sorted(err))))
    assert max(ratio.values()) < 1, (label, err, ratio)
    return ratio


def check_columns(label, b, got, wants, group):
    for c in range(2):
        check('{} column={}'.format(label, c), got[c], wants[c], b['flat'], b['masks'][c], b['specs'][c], b['rates'][c], group)


def assert_same_bits(a, b, keys):
    for c in range(len(a)):
        for key in keys:
            assert same_bits(a[c][key], b[c][key]), (c, key)


def joint_launches(plan):
    """(op, count) of the plan's eigen launches, all of which must be of the vector-unit joint family."""
    assert eigen_families(plan) == {FAMILY['EIG_JOINT']}, plan
    eig = (OP['OP_EIG_TIPS'], OP['OP_EIG_LEVEL'], OP['OP_EIG_NARROW'], OP['OP_EIG_TIER'])
    return [(o, count) for o, _, count in plan if o in eig]


def expected_joint_launches(flat, k):
    """What pml_plan_bottom_up lists for a forest without tiers: the tips, a launch per level while wider than the narrow limit of
    4 x (64 / k) nodes, counted from the root end, and one launch for those at most that wide if there are two or more."""
    widths = [int(w) for w in np.diff(flat.bu_offsets)]
    tail = 0
    while tail < len(widths) and widths[len(widths) - 1 - tail] <= cases.joint_narrow_limit(k):
        tail += 1
    if tail < 2:
        tail = 0
    return [(OP['OP_EIG_TIPS'], 0)] + [(OP['OP_EIG_LEVEL'], w) for w in widths[:len(widths) - tail]] + (
        [(OP['OP_EIG_NARROW'], tail)] if tail else [])


@pytest.mark.parametrize('k', cases.STATES_TWO_MATRICES)
def test_every_state_count_on_forest_s(k, capfd):
    """
    Default switches: the lean kernel of the observed tips (column 1: plus the list it leaves to the general kernel, through the
    atomic counter), and the narrow launch; beyond 32 states the cherries' level, wider than 4 nodes, is a level launch of the plain
    loop as well.  The plan is the one the forest's level widths give, per k.  Beyond 32 states a second engine takes the tips in
    chunks of two passes (EIGJ_TIP_BLOCKS=1: 40 tips over 32 waves): tips are independent, so ln L and the tables keep their bits.
    """
    b = cases.build_joint(k, 'S')
    flat = b['flat']
    assert np.all(b['masks'][0][flat.is_tip].sum(axis=1) == 1) and not np.all(b['masks'][1][flat.is_tip].sum(axis=1) == 1)
    wants = [cases.joint_exact(k, 'S', c) for c in range(2)]
    for want in wants:
        precondition(want)
    got, plan = run_joint(flat, k, b['specs'], b['rates'], b['masks'], capfd)
    launches = joint_launches(plan)
    assert launches == expected_joint_launches(flat, k), plan
    assert has(plan, 'OP_EIG_TIPS', 'EIG_JOINT', 0) and has(plan, 'OP_EIG_NARROW', 'EIG_JOINT', 2), plan
    if k >= 33:   # (the limit is 4 nodes: the level of the cherries is a level launch at every one of these k)
        assert has(plan, 'OP_EIG_LEVEL', 'EIG_JOINT', 5), plan
    check_columns('k={} forest=S'.format(k), b, got, wants, group_of(k))
    if k >= 33:
        assert cases.j_tip_chunk_passes(k, flat.n_tips, 1024) == 1 and cases.j_tip_chunk_passes(k, flat.n_tips) == 2
        chunked, plan2 = run_joint(flat, k, b['specs'], b['rates'], b['masks'], capfd, dict(EIGJ_TIP_BLOCKS=1))
        assert joint_launches(plan2) == launches
        assert_same_bits(got, chunked, ('loglik', 'table'))


@pytest.mark.parametrize('k', cases.STATES_TWO_MATRICES)
def test_every_state_count_in_a_level_launch(k, capfd):
    """
    Forest J(k): n cherries under 2 nodes under a root -- one level launch over the cherries, the narrow launch above.  Up to 32
    states with EIGJ_BLOCKS=1, EIGJ_TIP_BLOCKS=1: 32 waves, three passes of the pipelined kernel in wave 0 (prologue, steady state,
    last), a last pass of a single node in wave 1, and tip chunks of several passes (cases.j_cherries has the grid arithmetic,
    cases.j_passes and j_tip_chunk_passes restate it and are asserted here: the plan names the launch, not its passes).  A second
    engine with NO_EIGJ_PIPE=1 runs the plain loop: same bits of ln L, tables, vectors, exponents and states.  Beyond 32 states 6
    cherries, one per wave, in two workgroups of the plain loop.
    """
    b = cases.build_joint(k, 'J')
    flat = b['flat']
    n = cases.j_cherries(k)
    assert [int(w) for w in np.diff(flat.bu_offsets)] == [n, 2, 1] and n > cases.joint_narrow_limit(k)
    tune = None
    if k <= 32:
        tune = cases.J_TUNE
        assert cases.j_passes(k, n) == (3, 1) and cases.j_tip_chunk_passes(k, flat.n_tips) > 1
    wants = [cases.joint_exact(k, 'J', c) for c in range(2)]
    for want in wants:
        precondition(want)
    got, plan = run_joint(flat, k, b['specs'], b['rates'], b['masks'], capfd, tune)
    assert joint_launches(plan) == [(OP['OP_EIG_TIPS'], 0), (OP['OP_EIG_LEVEL'], n), (OP['OP_EIG_NARROW'], 2)], plan
    assert (OP['OP_EIG_LEVEL'], FAMILY['EIG_JOINT'], n) in plan
    check_columns('k={} forest=J n={}'.format(k, n), b, got, wants, group_of(k))
    if k <= 32:
        plain, plan2 = run_joint(flat, k, b['specs'], b['rates'], b['masks'], capfd, dict(tune, NO_EIGJ_PIPE=1))
        assert joint_launches(plan2) == joint_launches(plan)
        assert_same_bits(got, plain, ('loglik', 'table', 'bu', 'bu_sf', 'states'))


@pytest.mark.parametrize('k', [5, 20, 32])
def test_general_tips_kernel_alone(k, capfd):
    """EIGJ_ONE_TIPS_KERNEL=1 on forest S: every tip in eigen_joint_tips_kernel, whose passes of observed tips take its own closed
    form -- (A e) A^-1 where the lean kernel has A (e A^-1): other rounding, so held to the exact pass, not to the lean kernel's bits."""
    b = cases.build_joint(k, 'S')
    wants = [cases.joint_exact(k, 'S', c) for c in range(2)]
    for want in wants:
        precondition(want)
    got, plan = run_joint(b['flat'], k, b['specs'], b['rates'], b['masks'], capfd, dict(EIGJ_ONE_TIPS_KERNEL=1))
    assert joint_launches(plan) == expected_joint_launches(b['flat'], k), plan
    check_columns('k={} forest=S one tips kernel'.format(k), b, got, wants, 'valu32')


def took_joint_valu(plan):
    joint_launches(plan)


def took_hky_in_registers(plan):
    """Plain level launches WITHOUT the per-branch pass: P(t) is built in registers."""
    assert not has(plan, 'OP_PREP', None, 0) and has(plan, 'OP_LEVEL'), plan
    assert not eigen_families(plan), plan


def took_materialised(plan):
    """bu_matrix_kernel in joint mode on P(t) in HBM: the per-branch pass and plain level launches, no eigen launch."""
    assert has(plan, 'OP_PREP', None, 0) and has(plan, 'OP_LEVEL'), plan
    assert not eigen_families(plan), plan


def took_fused_matrix_core(plan):
    assert eigen_families(plan) == {FAMILY['EIG_FUSED']}, plan


DEEP = [('EIGEN', 11, took_joint_valu, 'valu32'), ('EIGEN', 20, took_joint_valu, 'valu32'), ('EIGEN', 43, took_joint_valu, 'valu64'),
        ('HKY', 4, took_hky_in_registers, 'other')]


@pytest.mark.parametrize('kind,k,took,group', DEEP, ids=['{}{}'.format(d[0], d[1]) for d in DEEP])
def test_rescaling_on_a_deep_caterpillar(kind, k, took, group, capfd):
    """One observed tip per level, as deep as takes the exact SUM vector of the root below 2^-800; the max-product vector lies below
    it entry by entry, so it is below 2^-800 too (asserted): four trips through the rescaling band at least, in the shuffle over one
    node's lanes of eigj_front_finish (npw 5, 3, 1) and in the joint mode of pml_kernels_matrix.h."""
    d = cases.deep_caterpillar(kind, k)
    want = cases.deep_joint_exact(kind, k)
    precondition(want)
    assert want['bu_log10'][0].max() * exact.LOG2_OF_10 < cases.DEEP_LOG2
    got, plan = run_joint(d['flat'], k, [d['spec']], [d['rates']], d['masks'][None], capfd)
    took(plan)
    check('deep {} k={} depth={}'.format(kind, k, d['depth']), got[0], want, d['flat'], d['masks'], d['spec'], d['rates'], group)
    inner = np.array(d['spine'][1:-1])
    assert np.any(got[0]['bu_sf'][inner] != 0), 'no rescaling on the spine'
    print('joint-shapes deep {} k={}: {} distinct scales on the spine'.format(kind, k, len(np.unique(got[0]['bu_sf'][inner]))))


@pytest.mark.parametrize('k', [5, 20])
def test_rescaling_inside_a_level_launch(k, capfd):
    """140 polytomies of observed tips in rare states on long branches, one level above the narrow limit: a level launch of the
    pipelined kernel whose product leaves the band inside the loop over the children, at npw = 12 and 3 (the maximum over a node's
    lanes comes through __shfl over that node's lanes only)."""
    d = cases.polytomy_forest(k)
    want = cases.polytomy_joint_exact(k)
    precondition(want)
    assert np.all(want['bu_log10'][d['polytomies']].max(axis=1) * exact.LOG2_OF_10 < -200)
    got, plan = run_joint(d['flat'], k, [d['spec']], [d['rates']], d['masks'][None], capfd)
    n = len(d['polytomies'])
    assert joint_launches(plan) == [(OP['OP_EIG_TIPS'], 0), (OP['OP_EIG_LEVEL'], n), (OP['OP_EIG_LEVEL'], n)], plan
    check('polytomies k={} fan={}'.format(k, d['fan']), got[0], want, d['flat'], d['masks'], d['spec'], d['rates'], 'valu32')
    assert np.all(got[0]['bu_sf'][d['polytomies']] != 0), 'no rescaling on the level of the polytomies'


@pytest.mark.parametrize('which', ['S', 'J'])
def test_hky_joint_sweep(which, capfd):
    """HKY (4 states, P(t) in registers) on forest S and on a J-shaped forest of 258 cherries, a level above the plain narrow limit
    of 256 units at two columns: plain level launches."""
    b = cases.build_joint(4, which, 'HKY')
    wants = [cases.joint_exact(4, which, c, 'HKY') for c in range(2)]
    for want in wants:
        precondition(want)
    got, plan = run_joint(b['flat'], 4, b['specs'], b['rates'], b['masks'], capfd)
    took_hky_in_registers(plan)
    if which == 'J':
        assert any(o == OP['OP_LEVEL'] and count == cases.HKY_J_CHERRIES for o, _, count in plan), plan
    check_columns('HKY forest={}'.format(which), b, got, wants, 'other')


NO_VALU = [(5, took_materialised), (20, took_fused_matrix_core), (40, took_materialised)]


@pytest.mark.parametrize('k,took', NO_VALU, ids=[str(d[0]) for d in NO_VALU])
def test_joint_sweep_without_the_vector_unit_kernels(k, took, capfd):
    """NO_EIGEN_JOINT_VALU=1 on forest S: bu_matrix_kernel on materialised P(t) with one state per lane (5) and two (40), and the
    fused matrix-core sweep (20, pml_kernels_eigen_mfma.h)."""
    b = cases.build_joint(k, 'S')
    wants = [cases.joint_exact(k, 'S', c) for c in range(2)]
    for want in wants:
        precondition(want)
    got, plan = run_joint(b['flat'], k, b['specs'], b['rates'], b['masks'], capfd, dict(NO_EIGEN_JOINT_VALU=1))
    took(plan)
    assert FAMILY['EIG_JOINT'] not in eigen_families(plan)
    check_columns('k={} forest=S NO_EIGEN_JOINT_VALU'.format(k), b, got, wants, 'other')


@pytest.mark.parametrize('k', [65, 128, 129])
def test_joint_sweep_beyond_64_states(k, capfd):
    """The production path beyond 64 states on forest T: bu_matrix_kernel in joint mode on P(t) from pij_eigen_wide_kernel, at both
    of its lane groups (up to 128 states, and beyond)."""
    b = cases.build_joint(k, 'T')
    wants = [cases.joint_exact(k, 'T', c) for c in range(2)]
    for want in wants:
        precondition(want)
    got, plan = run_joint(b['flat'], k, b['specs'], b['rates'], b['masks'], capfd)
    took_materialised(plan)
    check_columns('k={} forest=T'.format(k), b, got, wants, 'other')
