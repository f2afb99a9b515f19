"""The posterior rows of observed tips stay in memory across marginal passes (PmlResults::tip_rows_kept).

An observed tip's posterior row is the unit vector of its mask's one state: it depends on the masks and on nothing else.  The F81
kernels of one mask word leave its store out while the library can prove that the row stands -- and the table a caller sees must
be, bit for bit, the table of a pass that writes every row: here against an engine with PASTML_HIP_NO_KEEP_TIP_ROWS set, or
against a fresh engine that runs the last pass alone.  All comparisons are np.array_equal(..., equal_nan=True) on full downloads
of the posteriors, the likelihood sums, their scales, and on ln L.  Nothing here profiles, so the captured graphs replay.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from pastml_amd import hip, synthetic
from pastml_amd.tree import FlatForest
from test_gpu_parity import LEVEL_SCHEDULE, _forest_with_balanced_clumps, random_masks, random_spec

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
C = 3
OFF = dict(NO_KEEP_TIP_ROWS=1)
FORESTS = ('single', 'blocks', 'levels_balanced', 'levels_clumps')


def forest_of(name):
    """(forest, the tunables that select its schedule, the schedule pml_sweep_schedule must report)."""
    if name == 'single':
        return synthetic.balanced_forest(6), {}, (hip.SCHEDULE_SINGLE_LAUNCH,)
    if name == 'blocks':
        return (FlatForest.random(500, seed=31, max_arity=3, zero_frac=0.0, n_trees=2), dict(SMALL_MAX_NODES=0, BLOCK_NODES=32),   # (not one launch; blocks of 32 stored nodes)
                (hip.SCHEDULE_BLOCKS,))
    if name == 'levels_balanced':
        return synthetic.balanced_forest(12), dict(LEVEL_SCHEDULE), (hip.SCHEDULE_TWO_LEVEL, hip.SCHEDULE_LEVELS)
    return (_forest_with_balanced_clumps(700, seed=5), dict(LEVEL_SCHEDULE, SMALL_MAX_NODES=0),
            (hip.SCHEDULE_TWO_LEVEL, hip.SCHEDULE_LEVELS))


def inputs_of(name, k, n_passes=4):
    """Masks with observed, ambiguous and unknown tips (column 0: every tip observed) and n_passes different parameter sets."""
    flat, tune, schedules = forest_of(name)
    rng = np.random.default_rng(7000 + 13 * k + FORESTS.index(name))
    masks = np.stack([random_masks(flat, k, rng) for _ in range(C)])
    masks[0] = synthetic.one_hot_masks(flat, k, rng.integers(0, k, size=flat.n_tips))
    params = [[(random_spec('F81', k, rng), (float(rng.uniform(0.4, 3)), 0.0, 1.0)) for _ in range(C)] for _ in range(n_passes)]
    return flat, tune, schedules, masks, params


def tables(eng, lnl):
    """ln L and the three tables of every column, as full downloads."""
    return (np.array(lnl),) + tuple(np.stack([eng.download(what, c) for c in range(eng.n_cols)])
                                    for what in (hip.BUF_POSTERIOR, hip.BUF_LH_SUM, hip.BUF_LH_SF))


def one_pass(eng, models):
    eng.set_models(models)
    lnl, _, _, _ = eng.marginal_pass(posterior=False, lh=False)   # (nothing to copy: the pass may end in the spin on its word)
    return tables(eng, lnl)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def fresh_tables(flat, k, tune, masks, models, n_cols=C):
    with hip.Engine(flat, n_cols, k, tune=tune) as eng:
        eng.set_masks(masks)
        return one_pass(eng, models)


# ---------------------------------------------------------------------------------------------------------------------
CHILD = '''
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
from pastml_amd import hip
import test_gpu_tip_rows_kept as t
out = dict()
for name in t.FORESTS:
    for k in (4, 20, 64):
        flat, tune, schedules, masks, params = t.inputs_of(name, k)
        with hip.Engine(flat, t.C, k, tune=tune) as eng:
            eng.set_masks(masks)
            assert eng.sweep_schedule()[0] in schedules, (name, k, eng.sweep_schedule())
            for i in range(3):
                sys.stderr.write('CASE {{}} {{}} PASS {{}}\\n'.format(name, k, i)); sys.stderr.flush()
                for j, a in enumerate(t.one_pass(eng, params[i])):
                    out['{{}}_{{}}_{{}}_{{}}'.format(name, k, i, j)] = a
        sys.stderr.write('CASE end\\n'); sys.stderr.flush()
np.savez({npz!r}, **out)
'''


@pytest.fixture(scope='module')
def kept_runs(tmp_path_factory):
    """Three passes with different parameters on every schedule and k, by the default engine in a child process that runs with
    PASTML_HIP_DEBUG=1: (the tables after every pass, what the library said about the tips' rows in every pass)."""
    npz = str(tmp_path_factory.mktemp('kept') / 'kept.npz')
    env = dict(os.environ, PASTML_HIP_DEBUG='1')
    res = subprocess.run([sys.executable, '-c', CHILD.format(root=REPO, tests=HERE, npz=npz)], env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    said, case = dict(), None
    for line in res.stderr.splitlines():
        if line.startswith('CASE '):
            w = line.split()
            case = (w[1], int(w[2]), int(w[4])) if len(w) == 5 else None
        elif case is not None and line.startswith("pml plan: top-down sweep, observed tips' rows "):
            said.setdefault(case, set()).add(line.rsplit(' ', 1)[1])
    return np.load(npz), said


@pytest.mark.parametrize('k', [4, 20, 64])
@pytest.mark.parametrize('name', FORESTS)
def test_every_schedule_keeps_the_rows_and_gives_the_same_table(kept_runs, name, k):
    """Single launch, subtree blocks, level schedule with two-level and stacked units (a balanced tree, a forest with balanced
    clumps); observed, ambiguous and unknown tips and one column with every tip observed; three passes with different
    parameters.  After every pass the default engine's tables are those of the engine with the off switch, and in passes two
    and three the library says that the rows were kept (in the first, that they were written)."""
    kept, said = kept_runs
    flat, tune, schedules, masks, params = inputs_of(name, k)
    with hip.Engine(flat, C, k, tune=dict(tune, **OFF)) as eng:
        eng.set_masks(masks)
        assert eng.sweep_schedule()[0] in schedules
        if name.startswith('levels') and k >= 17:   # (two-level and stacked units take 8 lanes and more per unit)
            on, n_two, n_stack = eng.schedule_info()
            assert on and n_two > 0 and n_stack > 0, (on, n_two, n_stack)
        for i in range(3):
            want = one_pass(eng, params[i])
            got = tuple(kept['{}_{}_{}_{}'.format(name, k, i, j)] for j in range(4))
            assert same(got, want), (name, k, i)
            assert np.isfinite(want[1]).all()
    assert [said.get((name, k, i)) for i in range(3)] == [{'written'}, {'kept'}, {'kept'}], said


# ---------------------------------------------------------------------------------------------------------------------
def _upload_again(eng):
    """pml_tree_upload and pml_chars_alloc once more on the engine's context (Engine.__init__'s calls): the columns, and with
    them the posterior table, are allocated anew."""
    flat, i32 = eng.flat, ctypes.c_int32
    a = {n: np.ascontiguousarray(getattr(flat, n), dtype=np.int32) for n in
         ('parent', 'first_child', 'n_children', 'bu_offsets', 'bu_order', 'td_offsets', 'td_parent_offsets', 'td_parents', 'post_rank')}
    dist = np.ascontiguousarray(flat.dist, dtype=np.float64)
    p = lambda x: x.ctypes.data_as(ctypes.POINTER(i32))   # noqa: E731
    hip._check(eng._lib.pml_tree_upload(eng._ctx, flat.n_nodes, len(flat.roots), p(a['parent']), p(a['first_child']), p(a['n_children']),
                                        dist.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), flat.n_bu_levels, p(a['bu_offsets']),
                                        p(a['bu_order']), flat.n_td_levels, p(a['td_offsets']), p(a['td_parent_offsets']),
                                        p(a['td_parents']), p(a['post_rank'])))
    hip._check(eng._lib.pml_chars_alloc(eng._ctx, eng.n_cols, eng.k))


ACTIONS = ('tip_states', 'masks', 'select', 'realloc', 'download_td', 'option')


@pytest.mark.parametrize('action', ACTIONS)
@pytest.mark.parametrize('name', ['single', 'levels_balanced'])
def test_whatever_may_touch_the_rows_makes_the_next_pass_write_them(name, action):
    """Three passes (the level schedule's third replays the graph its second captured, in skip mode), then one of: other tip
    states; masks that turn an observed tip ambiguous and give another one a different state; a MAP selection and the original
    masks again; the columns allocated anew; a download of the TD vectors (the lazy sweep with the stores on); the option that
    leaves the rows out of memory switched on and off again.  The pass after it gives the tables of a fresh engine that runs
    that pass alone -- on the level schedule by replaying the graph captured in skip mode, the stale-graph hazard -- and so does
    one more pass behind it, which keeps the rows again."""
    k = 20
    flat, tune, _, masks, params = inputs_of(name, k, n_passes=5)
    rng = np.random.default_rng(5)
    with hip.Engine(flat, C, k, tune=tune) as eng:
        eng.set_masks(masks)
        for i in range(3):
            one_pass(eng, params[i])
        now = masks
        if action == 'tip_states':
            states = rng.integers(0, k, size=(C, flat.n_tips))
            eng.set_tip_states(states)
            now = np.stack([synthetic.one_hot_masks(flat, k, s) for s in states])
        elif action == 'masks':
            now = masks.copy()
            tips = np.flatnonzero(flat.is_tip)
            a, b = tips[3], tips[len(tips) // 2]
            sa, sb = int(np.argmax(masks[0, a])), int(np.argmax(masks[0, b]))
            now[0, a, (sa + 1) % k] = 1            # observed -> ambiguous
            now[0, b] = 0
            now[0, b, (sb + 5) % k] = 1            # observed, another state
            eng.set_masks(now)
        elif action == 'select':
            eng.select_states('MAP')
            eng.set_masks(masks)
        elif action == 'realloc':
            _upload_again(eng)
            eng.set_masks(masks)
        elif action == 'download_td':
            eng.download(hip.BUF_TD, 1)
        elif action == 'option':
            eng.set_option(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)
            eng.set_option(hip.OPT_IMPLICIT_TIP_POSTERIORS, 0)
        for i in (3, 4):
            got = one_pass(eng, params[i])
            assert same(got, fresh_tables(flat, k, tune, now, params[i])), (name, action, i)


# ---------------------------------------------------------------------------------------------------------------------
def _observed_tip(flat, masks, col, which=7):
    tips = np.flatnonzero(flat.is_tip)
    tip = int(tips[np.flatnonzero(masks[col, tips].sum(axis=1) == 1)[which]])
    return tips, tip, int(np.argmax(masks[col, tip]))


def _with_pi_s(models, col, s, value):
    """The parameter set with pi_s = value in column col (the other frequencies rescaled)."""
    out = [(dict(spec, pi=spec['pi'].copy()), rates) for spec, rates in models]
    pi = out[col][0]['pi']
    pi[s] = 0.0
    pi /= pi.sum()
    pi[s] = value
    return out


def test_a_failed_pass_is_repaired_by_the_next_good_pass():
    """Column 1 has observed tips whose state s gets frequency pi_s = 0 in the second of three passes: that pass raises the zero
    likelihood as before (its tables are not to be had: the record holds no result), the first and the third run with healthy
    parameters.  After the first the tables are those of the off-switch engine; after the third, which must not count on rows
    the failed pass may have overwritten, those of the off-switch engine and of a fresh engine, the healthy columns' included."""
    k = 20
    flat, tune, _, masks, params = inputs_of('blocks', k)
    _, _, s = _observed_tip(flat, masks, 1)
    with hip.Engine(flat, C, k, tune=tune) as eng, hip.Engine(flat, C, k, tune=dict(tune, **OFF)) as off:
        eng.set_masks(masks)
        off.set_masks(masks)
        assert same(one_pass(eng, params[0]), one_pass(off, params[0]))
        for e in (eng, off):
            with pytest.raises(hip.ZeroLikelihoodError):
                one_pass(e, _with_pi_s(params[1], 1, s, 0.0))
        got = one_pass(eng, params[2])
        assert same(got, one_pass(off, params[2])) and same(got, fresh_tables(flat, k, tune, masks, params[2]))
        assert np.isfinite(got[1]).all()
        assert same(one_pass(eng, params[3]), one_pass(off, params[3]))   # (rows kept again)


def test_a_nan_row_is_repaired_by_the_next_good_pass():
    """
    f81_finish_tip_word writes NaNs for an observed tip when lhs = tds * pi_s is not a positive finite number, in a pass that
    returns no error.  That happens where c0 = (1 - e) pi_s is denormal: its reciprocal overflows, tds and lhs are inf.  Here
    one observed tip of column 1, the only tip of the column in its state s, sits on a branch of length 1e-5 (1 - e of that
    order) and pi_s = 1e-305 in the bad pass.  A good pass, the bad pass (no error; the tip's row is NaNs and equals the
    off-switch engine's NaN row; the healthy columns are finite), a good pass again: the row is the unit vector again and the
    tables are a fresh engine's -- the bad-tip word made that pass write every row.  Then the rows are kept again.
    An input whose ln L is finite at the root while a tip is not ok was not found at these sizes: on this one, and on the same
    forest with pi_s = 1e-310 or with sixteen tips in state s, the bad pass returns no error and ln L of column 1 is -inf (in both
    engines, bit for bit).  What the case is for holds all the same: the pass succeeds, the NaNs overwrite a kept unit row, and
    only the bad-tip word tells the host.
    """
    k = 20
    flat, tune, _, masks, params = inputs_of('blocks', k)
    tips, tip, s = _observed_tip(flat, masks, 1)
    flat.dist[tip] = 1e-5
    others = [n for n in tips if n != tip and masks[1, n, s]]   # no other tip of the column may be in state s
    masks[1, others, s] = 0
    masks[1, others, (s + 1) % k] = 1
    with hip.Engine(flat, C, k, tune=tune) as eng, hip.Engine(flat, C, k, tune=dict(tune, **OFF)) as off:
        eng.set_masks(masks)
        off.set_masks(masks)
        assert same(one_pass(eng, params[0]), one_pass(off, params[0]))
        bad = _with_pi_s(params[1], 1, s, 1e-305)
        got, want = one_pass(eng, bad), one_pass(off, bad)
        assert np.isfinite(want[0][[0, 2]]).all() and np.isnan(want[1][1, tip]).all(), (want[0], want[1][1, tip])
        assert np.isfinite(want[1][[0, 2]]).all()   # (the healthy columns)
        assert same(got, want)
        got = one_pass(eng, params[2])
        assert same(got, one_pass(off, params[2])) and same(got, fresh_tables(flat, k, tune, masks, params[2]))
        assert np.array_equal(got[1][1, tip], masks[1, tip].astype(float))
        assert same(one_pass(eng, params[3]), one_pass(off, params[3]))   # (rows kept again)


@pytest.mark.parametrize('kind,k', [('F81', 65), ('EIGEN', 5)])
def test_other_kernels_write_every_row(kind, k):
    """Two mask words (k = 65) and an eigen model: the mechanism is off, three passes give the tables of the off switch."""
    flat = FlatForest.random(500, seed=31, max_arity=3, zero_frac=0.0, n_trees=2)
    rng = np.random.default_rng(40 + k)
    masks = np.stack([random_masks(flat, k, rng) for _ in range(C)])
    masks[0] = synthetic.one_hot_masks(flat, k, rng.integers(0, k, size=flat.n_tips))
    params = [[(random_spec(kind, k, rng), (float(rng.uniform(0.4, 3)), 0.0, 1.0)) for _ in range(C)] for _ in range(3)]
    with hip.Engine(flat, C, k) as eng, hip.Engine(flat, C, k, tune=OFF) as off:
        eng.set_masks(masks)
        off.set_masks(masks)
        for i in range(3):
            got = one_pass(eng, params[i])
            assert same(got, one_pass(off, params[i])), i
            assert np.isfinite(got[1]).all()
