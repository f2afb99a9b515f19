"""What a context's result buffers hold (csrc/pml_results.h), through the call orders it governs: every refusal with its status and
its exact message, and every lazy materialisation -- the cherries, the children of the two-level and stacked units, the TD
vectors, the observed tips' posteriors -- written once and correctly: a buffer downloaded twice is the same array, and it is the
array of a context that never left those rows out.  Every sweep runs twice before anything is looked at (the second one replays
the captured launches where there are any).  Bitwise comparisons throughout."""
import numpy as np
import pytest

import optimiser_point_cases as cases
from oracle import pastml_oracle as orc
from pastml_amd import hip, synthetic
from pastml_amd.tree import FlatForest, TreeNode
from test_gpu_parity import LEVEL_SCHEDULE

pytestmark = pytest.mark.gpu

NO_TD = 'pml_top_down_marginals needs a successful marginal pml_bottom_up first'
NO_BACKTRACE = 'pml_joint_backtrace needs a successful joint pml_bottom_up first'
NO_TD_SWEEP = 'no valid top-down sweep'
NO_JOINT_STATES = 'no valid joint back-trace'
NO_PASS = '{} needs a marginal pml_bottom_up and pml_top_down_marginals first'
NO_SELECT = 'pml_select_states needs pml_top_down_marginals first'
K, C = 4, 3


def ragged_tree():
    """9 tips: a caterpillar of depth 5 whose side branches are a tip, a cherry, a tip, a cherry and, at the end, a cherry."""
    rng = np.random.default_rng(3)
    root = TreeNode(name='', dist=0.0)
    spine = root
    for side in (1, 2, 1, 2):
        sub = spine.add_child(dist=float(rng.uniform(0.01, 0.3)))
        if side == 2:
            for _ in range(2):
                sub.add_child(dist=float(rng.uniform(0.01, 0.3)))
        spine = spine.add_child(dist=float(rng.uniform(0.01, 0.3)))
    for _ in range(2):
        spine.add_child(dist=float(rng.uniform(0.01, 0.3)))
    return root


def cherry():
    root = TreeNode(name='', dist=0.0)
    root.add_child(dist=0.1)
    root.add_child(dist=0.25)
    return root


def named(roots):
    for ti, root in enumerate(roots):
        for i, n in enumerate(root.traverse('preorder')):
            n.name = 't{}_{}'.format(ti, i) if n.is_leaf() else 'n{}_{}'.format(ti, i)
    return FlatForest.from_trees(roots)


def f81_engine(flat, k=K, cols=C, options=(), **kwargs):
    eng = hip.Engine(flat, cols, k, **kwargs)
    for option, value in options:
        eng.set_option(option, value)
    eng.models = [(dict(kind=0, pi=synthetic.f81_frequencies(k, c)), (1.0 + 0.5 * c, 0.01, 0.9)) for c in range(cols)]   # (tau > 0: the clump forest has branches of length 0)
    eng.set_models(eng.models)
    eng.set_tip_states(tip_states(flat, k, cols))
    return eng


def tip_states(flat, k, cols):
    return np.stack([synthetic.tip_states(flat.n_tips, k, c) for c in range(cols)])


def eigen_engine(flat, k=20):
    rng = np.random.default_rng(0)
    pi = rng.dirichlet(np.ones(k) * 3)
    rates = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
    d, a, ainv = orc.diagonalise(pi, rates + rates.T)
    eng = hip.Engine(flat, 1, k)
    eng.models = [(dict(kind=2, pi=pi, d=d, A=a, Ainv=ainv), (1.0, 0.0, 1.0))]
    eng.set_models(eng.models)
    eng.set_tip_states(tip_states(flat, k, 1))
    return eng


def refused(call, message):
    with pytest.raises(hip.HipError) as e:
        call()
    assert e.value.status == hip.PML_ERR_INVALID, e.value
    assert str(e.value) == 'libpastml_hip: {} (status {})'.format(message, hip.PML_ERR_INVALID)


def downloads_refused(eng):
    refused(lambda: eng.download(hip.BUF_TD), NO_TD_SWEEP)
    refused(lambda: eng.download(hip.BUF_POSTERIOR), NO_TD_SWEEP)
    refused(lambda: eng.download(hip.BUF_JOINT_STATE), NO_JOINT_STATES)


def test_refusals_before_the_sweeps():
    flat = named([ragged_tree(), cherry()])
    with f81_engine(flat) as eng:
        refused(eng.top_down_marginals, NO_TD)
        refused(eng.joint_backtrace, NO_BACKTRACE)
        downloads_refused(eng)
        refused(lambda: eng.select_states('MAP'), NO_SELECT)
        eng.bottom_up(False)
        refused(eng.top_down_marginals, NO_TD)   # (a joint sweep is no marginal one)
        eng.bottom_up(True)
        refused(eng.joint_backtrace, NO_BACKTRACE)
        refused(lambda: eng.marginal_counts(4, 1), NO_PASS.format('pml_marginal_counts'))
        refused(eng.expected_counts, NO_PASS.format('pml_expected_counts'))
        refused(lambda: eng.sample_scenarios(4, 1), NO_PASS.format('pml_sample_scenarios'))
        refused(lambda: eng.select_states('MAP'), NO_SELECT)
        downloads_refused(eng)
        eng.top_down_marginals()
        assert eng.marginal_counts(4, 1).shape == (K, K) and eng.expected_counts().shape == (C, K, K)
        assert eng.sample_scenarios(4, 1)[0].shape == (flat.n_nodes, 4)


def input_changes(eng, flat, eigen):
    """The calls after which no sweep's result stands (each changes something every time it is called)."""
    fused = [1]

    def flip_eigen_fused():
        fused[0] ^= 1
        eng.set_option(hip.OPT_EIGEN_FUSED, fused[0])

    changes = [lambda: eng.set_models(eng.models), lambda: eng.set_tip_states(tip_states(flat, eng.k, eng.n_cols)),
               lambda: eng.set_tunable('NO_SPIN_WAIT', 1)]
    return changes + ([flip_eigen_fused] if eigen else [])


@pytest.mark.parametrize('eigen', [False, True])
def test_refusals_after_the_inputs_changed(eigen):
    flat = named([ragged_tree()] + ([] if eigen else [cherry()]))
    with (eigen_engine(flat) if eigen else f81_engine(flat)) as eng:
        for change in input_changes(eng, flat, eigen):
            eng.marginal_pass()
            eng.download(hip.BUF_TD), eng.download(hip.BUF_POSTERIOR)   # served ...
            change()
            downloads_refused(eng)   # ... and no longer
            refused(eng.top_down_marginals, NO_TD)
            eng.joint_pass()
            eng.download(hip.BUF_JOINT_STATE)
            change()
            downloads_refused(eng)
            refused(eng.joint_backtrace, NO_BACKTRACE)


def test_selection_keeps_the_posteriors():
    flat = named([ragged_tree(), cherry()])
    with f81_engine(flat) as eng:
        eng.marginal_pass()
        post = [eng.download(hip.BUF_POSTERIOR, c) for c in range(C)]
        eng.select_states('MAP')
        for c in range(C):
            assert np.array_equal(eng.download(hip.BUF_POSTERIOR, c), post[c])
        refused(eng.top_down_marginals, NO_TD)
        eng.bottom_up(True)
        eng.top_down_marginals()


def looked_at(eng, some_columns):
    """Every sweep twice, then each buffer of each column twice: {(buffer, column): array}."""
    for _ in range(2):
        eng.marginal_pass(posterior=False, lh=False)
    if some_columns:
        active = np.array([1, 0, 1], dtype=np.uint8)
        for _ in range(2):
            eng.bottom_up_submit(True, active)
            eng.bottom_up_collect(True)
        for _ in range(2):
            eng.top_down_marginals(posterior=False, lh=False)
    got = {}
    for what in (hip.BUF_BU, hip.BUF_TD, hip.BUF_POSTERIOR):
        for c in range(eng.n_cols):
            got[what, c] = eng.download(what, c)
            assert np.array_equal(eng.download(what, c), got[what, c]), (what, c)
    return got


# (forest, states, switches; two-level and stacked units take 8 lanes and more per unit: 20 states)
SCHEDULES = {'single launch': (lambda: named([ragged_tree(), cherry()]), K, None),
             'levels': (lambda: cases.forest('clumps')[0], 20, dict(LEVEL_SCHEDULE, SMALL_MAX_NODES=0))}


@pytest.mark.parametrize('some_columns', [False, True])
@pytest.mark.parametrize('schedule', sorted(SCHEDULES))
def test_rows_left_out_are_written_once(schedule, some_columns):
    make, k, tune = SCHEDULES[schedule]
    flat = make()
    with f81_engine(flat, k, tune=tune) as eng:
        if schedule == 'levels':   # (the only schedule that leaves the children of two-level and stacked units out of memory)
            on, n_two, n_stacked = eng.schedule_info()
            assert on and n_two > 0 and n_stacked > 0, (on, n_two, n_stacked)
        got = looked_at(eng, some_columns)
    # the same calls on contexts that write those rows in the sweep itself
    variants = {hip.BUF_BU: dict(cherry_fusion=False), hip.BUF_TD: dict(keep_td=True),
                hip.BUF_POSTERIOR: dict(options=[(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)])}
    for what, kwargs in variants.items():
        with f81_engine(flat, k, tune=tune, **kwargs) as other:
            theirs = looked_at(other, some_columns)
        rows = flat.parent >= 0 if what == hip.BUF_TD else slice(None)   # (a root has no top-down vector)
        for c in range(C):
            assert np.array_equal(got[what, c][rows], theirs[what, c][rows]), (what, c)


def test_joint_sweep_of_an_eigen_context():
    flat = named([ragged_tree()])
    with eigen_engine(flat) as eng:
        refused(eng.joint_backtrace, NO_BACKTRACE)
        for _ in range(2):
            lnl, states = eng.joint_pass()
        assert np.array_equal(eng.download(hip.BUF_JOINT_STATE), states[0])
        bu = eng.download(hip.BUF_BU)
        assert np.array_equal(eng.download(hip.BUF_BU), bu)
        refused(eng.top_down_marginals, NO_TD)
        refused(lambda: eng.download(hip.BUF_POSTERIOR), NO_TD_SWEEP)
        eng.bottom_up(True)
        refused(eng.joint_backtrace, NO_BACKTRACE)
        refused(lambda: eng.download(hip.BUF_JOINT_STATE), NO_JOINT_STATES)
