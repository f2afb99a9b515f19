"""
The entries that read what a marginal pass left on the device (Reader::rows, pml_api_readers.hip, and pml_select_states) on the
schedules that leave rows out of memory: two-level and stacked units and the two chained launches, 17 <= k <= 64.  There the
cherries' bottom-up vectors, the children of the two-level and of the stacked units and the observed tips' posterior rows are
filled in lazily, by the first entry that needs them.

A  every consumer, as the first thing that touches a fresh context after marginal_pass(posterior=False, lh=False) -- no download
   before it, which would run the same materialisation --, against its reference with the checker and the tolerance of its own
   test file (imported, not restated): loglik_gradient, expected_history (+ identities), history_through_time (5 bins, one
   empty), expected_counts, sample_scenarios draw for draw, select_states MAP / MPPA / MPPA with force_joint.
B  the same bits as a context that stores every row (no cherry fusion, NO_SUPER, NO_STACK; schedule_info() says it has no units),
   for the four exact consumers and the five samplers, with each chain switched off as well.
C  call orders: new parameters between two passes; the replayed pass; downloads between two calls of a consumer; implicit tip
   rows; kept tip rows; a sweep of a column subset; a joint pass in between.

The forests, columns and references are tests/unit_schedule_cases.py's; tests/test_unit_schedule_cases_host.py holds every column
to a finite ln L, so nothing is skipped or filtered here.  chained is balanced_forest(7) at every k: the launch counts of the
profile say that both chains run there (16 two-level nodes, 5 stacked), as test_gpu_bu_chain.py::test_a_part_filled_tile has it
at k = 64.  Every case of A prints a line 'unit-schedules | ...' with its unit counts, its launch counts and the worst error /
tolerance per consumer; profiles/consumers_on_unit_schedules.txt is that table from an MI355X.
"""
import numpy as np
import pytest

import expected_history_ref as href
import test_gpu_bu_chain as bu_chain
import test_gpu_expected_counts as tcounts
import test_gpu_expected_history as thistory
import test_gpu_history_time as ttime
import test_gpu_loglik_gradient as tgradient
import test_gpu_scenarios as tscenarios
import test_gpu_td_chain as td_chain
import unit_schedule_cases as units
from pastml_amd import hip, ml

pytestmark = pytest.mark.gpu

N_SAMPLES = 64
SEED = (7 << 32) + 4242
NO_CHAINS = dict(NO_TD_CHAIN=1, NO_BU_CHAIN=1)
NEED_PASS = 'needs a marginal pml_bottom_up and pml_top_down_marginals first'


@pytest.fixture(autouse=True)
def references_once(monkeypatch):
    """The imported checkers compute their references through unit_schedule_cases.once: once per process and column."""
    for module, name, kept in units.REFERENCES:
        monkeypatch.setattr(module, name, kept)


# ---------------------------------------------------------------------------------------------------------------------
# contexts
# ---------------------------------------------------------------------------------------------------------------------

def engine(name, k, C=None, tune=None, storing=False, options=()):
    """A fresh context with the masks set.  With units: schedule_info() has to show two-level and stacked units; storing: none."""
    C = C or units.N_COLUMNS[name]
    tune = dict(units.TUNE, **(tune or {}))
    if storing:
        eng = hip.Engine(units.forest(name), C, k, cherry_fusion=False, tune=dict(tune, NO_SUPER=1, NO_STACK=1))
    else:
        eng = hip.Engine(units.forest(name), C, k, tune=tune)
    try:
        scheduled, n_two, n_stacked = eng.schedule_info()
        if storing:
            assert n_two == 0 and n_stacked == 0, (scheduled, n_two, n_stacked)
        else:
            assert scheduled and n_two > 0 and n_stacked > 0, (scheduled, n_two, n_stacked)
        for option, value in options:
            eng.set_option(option, value)
        eng.set_masks(units.masks(name, k)[:C])
    except Exception:
        eng.close()
        raise
    return eng


def one_pass(eng, models):
    eng.set_models(models[:eng.n_cols])
    lnl = eng.marginal_pass(posterior=False, lh=False)[0]
    assert np.isfinite(lnl).all(), lnl
    return lnl


def launches(name, k, tune=None):
    """(schedule_info, the launch counts of the profile's five brackets) of one marginal pass."""
    with engine(name, k, tune=tune) as eng:
        eng.set_models(units.models(name, k))
        _, counts = bu_chain.counted(eng, lambda: eng.marginal_pass(posterior=False, lh=False)[0])
        return eng.schedule_info(), counts


# ---------------------------------------------------------------------------------------------------------------------
# consumers
# ---------------------------------------------------------------------------------------------------------------------

EXACT = dict(
    gradient=lambda eng, name: eng.loglik_gradient(),
    history=lambda eng, name: eng.expected_history(jumps=True, branch_jumps=True),
    time=lambda eng, name: eng.history_through_time(units.node_times(name), units.boundaries(name)),
    counts=lambda eng, name: (eng.expected_counts(),))


def _per_column(eng, call):
    """A sampler's outputs of every column, stacked output by output."""
    got = [call(c) for c in range(eng.n_cols)]
    return tuple(np.stack([np.asarray(g[i]) for g in got]) for i in range(len(got[0])))


SAMPLERS = dict(
    scenarios=lambda eng, name: _per_column(eng, lambda c: eng.sample_scenarios(N_SAMPLES, SEED + c, col=c)),
    histories=lambda eng, name: _per_column(eng, lambda c: eng.sample_histories(N_SAMPLES, SEED + c, col=c, branch_jumps=True)),
    histories_time=lambda eng, name: _per_column(eng, lambda c: eng.sample_histories_through_time(
        units.node_times(name), units.boundaries(name), N_SAMPLES, SEED + c, col=c)),
    marginal_counts=lambda eng, name: _per_column(eng, lambda c: (eng.marginal_counts(N_SAMPLES, SEED + c, col=c),)),
    marginal_counts_altered=lambda eng, name: _per_column(eng, lambda c: eng.marginal_counts_altered(
        N_SAMPLES, SEED + c, units.altered(name), col=c)))
CONSUMERS = dict(EXACT, **SAMPLERS)


def consume(eng, name, which=None, posteriors=True):
    """{consumer: its outputs over all columns}, called in the order of ``which`` (default: all nine); with ``posteriors`` the
    downloaded posteriors [C, N, k] as well, after the last consumer."""
    out = {key: CONSUMERS[key](eng, name) for key in (which or CONSUMERS)}
    if posteriors:
        out['posteriors'] = (np.stack([eng.download(hip.BUF_POSTERIOR, c) for c in range(eng.n_cols)]),)
    return out


def same(a, b):
    """Tuples of arrays with the same shapes, types and bytes (every 64-bit word, NaNs included)."""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and
                                    np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def assert_same(got, want, label, keys=None, cols=None):
    for key in keys or want:
        a, b = got[key], want[key]
        if cols is not None:
            a, b = [x[cols] for x in a], [x[cols] for x in b]
        assert same(a, b), (label, key)


# ---------------------------------------------------------------------------------------------------------------------
# the four exact consumers against their references: the checkers of their own test files
# ---------------------------------------------------------------------------------------------------------------------

def _counts_ratio(got, want, n_branches):
    off = ~np.eye(want.shape[0], dtype=bool)
    err = np.abs(got - want)
    return max((err[off] / (1e-9 * np.abs(want[off]) + 1e-300)).max(), (err[~off] / (1e-9 * np.abs(want[~off]) + 1e-9 * n_branches)).max())


def check_exact(results, name, k, models, label, cols=None):
    """{consumer: worst error / tolerance over the columns}; every column is held by the checker of the consumer's own tests.
    models: what each column's last sweep ran with."""
    flat, masks = units.forest(name), units.masks(name, k)
    t, bounds = units.node_times(name), units.boundaries(name)
    n_branches = flat.n_nodes - len(flat.roots)
    worst = dict.fromkeys(results.keys() & EXACT.keys(), 0.0)
    for c in (range(len(results['posteriors'][0])) if cols is None else cols):
        model = models[c]
        spec, (sf, tau, tf) = model
        where = '{} column {}'.format(label, c)
        if 'gradient' in results:
            d_rates, d_pi, n_flat = results['gradient']
            r = tgradient._ratios((d_rates[c], d_pi[c], n_flat[c]), flat, masks[c], model, where)
            assert r.max() <= tgradient.TOLERANCE, (where, r.max())
            worst['gradient'] = max(worst['gradient'], r.max() / tgradient.TOLERANCE)
        if 'history' in results:
            got = tuple(x[c] for x in results['history'])
            thistory._check(got, flat, masks[c], model, where, rows=None)
            thistory._check_identities(got, results['posteriors'][0][c], flat, model, where)
            h = href.history(flat, masks[c], spec['pi'], sf, tau, tf, jump_rows=None)
            r = max(href.relative_errors(got[0], h['times']).max(), href.relative_errors(got[2], h['branch_jumps']).max(),
                    max(href.relative_errors(got[1][i], h['jumps'][i]).max() for i in range(k)))
            worst['history'] = max(worst['history'], r / thistory.TOLERANCE)
        if 'time' in results:
            got = tuple(x[c] for x in results['time'])
            ref = ttime._check(got, flat, masks[c], model, t, bounds, where, rows=None, route=units.by_subdivision)
            assert (got[0][4] == 0).all() and (got[1][4] == 0).all() and (got[2][4:] == 0).all(), where   # (the empty bin)
            worst['time'] = max(worst['time'], max(ttime._ratios(got, ref)) / ttime.TOLERANCE)
        if 'counts' in results:
            got = results['counts'][0][c]
            want = tcounts._restated(flat, masks[c], spec, (sf, tau, tf))['counts']
            assert not np.isnan(got).any(), where
            tcounts._assert_close(got, want, n_branches, where)
            worst['counts'] = max(worst['counts'], _counts_ratio(got, want, n_branches))
    return worst


def mixed(base, other, columns):
    return [other[c] if c in columns else base[c] for c in range(len(base))]


# ---------------------------------------------------------------------------------------------------------------------
# A. every consumer first on a fresh context
# ---------------------------------------------------------------------------------------------------------------------

def _assert_schedule(name, k):
    """The units through schedule_info(), the chains through the launch counts, as chained() of the two chain tests reads them."""
    info, on = launches(name, k)
    _, td_off = launches(name, k, dict(NO_TD_CHAIN=1))
    _, bu_off = launches(name, k, dict(NO_BU_CHAIN=1))
    _, off = launches(name, k, NO_CHAINS)
    if name == 'chained':
        assert info[1:] == (16, 5), info
        assert td_chain.chained(on, td_off), (on, td_off)
        assert bu_chain.chained(on, bu_off), (on, bu_off)
        assert on[0] == off[0] - 1 and on[1] == off[1] - 1 and on[2:] == off[2:] and on[3] == on[4] == 1, (on, off)
    else:
        assert on == td_off == bu_off == off and on[3] == on[4] == 1, (on, td_off, bu_off, off)
    return info, on, off


@pytest.mark.parametrize('name, k', units.FOREST_KS)
def test_every_consumer_first_on_a_fresh_context(name, k):
    flat, masks, models = units.forest(name), units.masks(name, k), units.models(name, k)
    C = len(models)
    label = '{} k={}'.format(name, k)
    info, on, off = _assert_schedule(name, k)
    ratios = {}
    for key in EXACT:
        with engine(name, k) as eng:
            one_pass(eng, models)
            results = consume(eng, name, which=[key])
        ratios.update(check_exact(results, name, k, models, label))
    # the scenarios draw for draw; the bottom-up vectors and posteriors the restatement needs come down after the sampling
    with engine(name, k) as eng:
        one_pass(eng, models)
        drawn = [eng.sample_scenarios(N_SAMPLES, SEED + c, col=c) for c in range(C)]
        vectors = [tscenarios._vectors(eng, models[c][0], c) for c in range(C)]
    for c in range(C):
        tscenarios._check(flat, drawn[c][0], drawn[c][1], vectors[c], masks[c], models[c][0]['pi'], SEED + c, 0,
                          '{} column {}'.format(label, c))
    # the selection against its host restatement on the posteriors of a context of its own
    with engine(name, k) as eng:
        eng.set_models(models)
        post = eng.marginal_pass(posterior=True, lh=False)[1]
    assert np.isfinite(post).all()
    for method, force_joint in (('MAP', False), ('MPPA', False), ('MPPA', True)):
        with engine(name, k) as eng:
            eng.set_models(models)
            states = eng.joint_pass()[1] if force_joint else None
            eng.marginal_pass(posterior=False, lh=False)
            selected, n_selected = eng.select_states(method, force_joint=force_joint)
        for c in range(C):
            if method == 'MAP':
                want, n_want = ml.select_map(post[c]), np.ones(flat.n_nodes, dtype=int)
            else:
                want, n_want = ml.select_mppa(post[c], states[c].astype(np.int64) if force_joint else None)
            assert np.array_equal(n_selected[c], n_want), (label, method, force_joint, c)
            assert np.array_equal(selected[c], want), (label, method, force_joint, c)
    print('unit-schedules | {:7s} | k={:2d} | two-level {:3d} stacked {:3d} | launches {} chains off {} | '.format(
        name, k, info[1], info[2], on, off) + ' '.join('{} {:.3g}'.format(key, ratios[key]) for key in EXACT) +
        ' | scenarios and selections exact')


# ---------------------------------------------------------------------------------------------------------------------
# B. the same bits as a context that stores every row
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name, k', [(name, k) for name in ('chained', 'clumps') for k in (20, 64)])
def test_same_bits_as_a_context_that_stores_every_row(name, k):
    models = units.models(name, k)
    label = '{} k={}'.format(name, k)
    with engine(name, k, storing=True) as eng:
        one_pass(eng, models)
        want = consume(eng, name)
    assert all(np.isfinite(x).all() for key in EXACT for x in want[key]), label
    # each consumer as the first one of a context with units ...
    for key in CONSUMERS:
        with engine(name, k) as eng:
            one_pass(eng, models)
            assert_same(consume(eng, name, which=[key], posteriors=False), want, (label, 'first'), keys=[key])
    # ... and all of them, in two orders, with each chain off, both off, both on
    for i, tune in enumerate((dict(NO_TD_CHAIN=1), dict(NO_BU_CHAIN=1), NO_CHAINS, {})):
        order = list(CONSUMERS)[::-1] if i % 2 else list(CONSUMERS)
        with engine(name, k, tune=tune) as eng:
            one_pass(eng, models)
            assert_same(consume(eng, name, which=order), want, (label, tune))


# ---------------------------------------------------------------------------------------------------------------------
# C. call orders
# ---------------------------------------------------------------------------------------------------------------------

ORDER_CASES = [('chained', 20), ('clumps', 64)]
COLUMNS = 5


def both(name, k, **how):
    """A context with units and the storing one, made the same way."""
    return engine(name, k, C=COLUMNS, **how), engine(name, k, C=COLUMNS, storing=True, **how)


def held(results, want, name, k, models, label, cols=None):
    """The exact consumers of a context with units against the references, every consumer against the storing context driven
    through the same calls."""
    ratios = check_exact(results, name, k, models, label, cols)
    print('{}: '.format(label) + ' '.join('{} {:.3g}'.format(key, ratios[key]) for key in EXACT))
    assert_same(results, want, label)


@pytest.mark.parametrize('name, k', ORDER_CASES)
def test_new_parameters_between_two_passes(name, k):
    """Pass, consumers, set_models with other parameters, pass, consumers: the second results are the reference's at the new
    parameters (a flag of the first pass that survived would leave rows of the first pass in the tables)."""
    first, second = units.models(name, k, 0)[:COLUMNS], units.models(name, k, 1)[:COLUMNS]
    label = '{} k={} new parameters'.format(name, k)
    got = []
    for eng in both(name, k):
        with eng:
            one_pass(eng, first)
            a = consume(eng, name)
            one_pass(eng, second)
            got.append((a, consume(eng, name)))
    held(got[0][0], got[1][0], name, k, first, label + ', first pass')
    held(got[0][1], got[1][1], name, k, second, label + ', second pass')


@pytest.mark.parametrize('name, k', ORDER_CASES)
def test_the_replayed_pass(name, k):
    """The same pass twice -- the second replays the captured graph --, then the consumers."""
    models = units.models(name, k)[:COLUMNS]
    got = []
    for eng in both(name, k):
        with eng:
            one_pass(eng, models)
            one_pass(eng, models)
            got.append(consume(eng, name))
    held(got[0], got[1], name, k, models, '{} k={} replay'.format(name, k))


@pytest.mark.parametrize('name, k', ORDER_CASES)
def test_downloads_between_and_before_the_consumers(name, k):
    """Consumer, download(BUF_BU), download(BUF_POSTERIOR), consumer again: the same words; a second context downloads first:
    the same words again."""
    models = units.models(name, k)[:COLUMNS]
    label = '{} k={} downloads'.format(name, k)

    def downloads(eng):
        return tuple(np.stack([eng.download(what, c) for c in range(COLUMNS)]) for what in (hip.BUF_BU, hip.BUF_POSTERIOR))
    with engine(name, k, C=COLUMNS, storing=True) as eng:
        one_pass(eng, models)
        want = consume(eng, name)
        want_tables = downloads(eng)
    with engine(name, k, C=COLUMNS) as eng:
        one_pass(eng, models)
        first = consume(eng, name, posteriors=False)
        between = downloads(eng)
        again = consume(eng, name)
    with engine(name, k, C=COLUMNS) as eng:
        one_pass(eng, models)
        before = downloads(eng)
        after = consume(eng, name)
    held(again, want, name, k, models, label)
    assert_same(first, again, label, keys=list(CONSUMERS))
    assert_same(after, again, label)
    # what came down: a bottom-up vector is stored to within its power-of-two scaling, a posterior row bit for bit
    assert same(between, before), label
    assert same(between[1:], want_tables[1:]), label


@pytest.mark.parametrize('name, k', ORDER_CASES)
def test_implicit_tip_rows(name, k):
    """OPT_IMPLICIT_TIP_POSTERIORS = 1: the same words as without it."""
    models = units.models(name, k)[:COLUMNS]
    label = '{} k={} implicit tip rows'.format(name, k)
    with engine(name, k, C=COLUMNS) as eng:
        one_pass(eng, models)
        plain = consume(eng, name)
    got = []
    for eng in both(name, k, options=[(hip.OPT_IMPLICIT_TIP_POSTERIORS, 1)]):
        with eng:
            one_pass(eng, models)
            got.append(consume(eng, name))
    held(got[0], got[1], name, k, models, label)
    assert_same(got[0], plain, label)


@pytest.mark.parametrize('name, k', ORDER_CASES)
def test_kept_tip_rows(name, k):
    """Masks set once, a pass with the first parameters, a pass with the second: the observed tips' rows are kept, not rewritten;
    with NO_KEEP_TIP_ROWS the same words."""
    first, second = units.models(name, k, 0)[:COLUMNS], units.models(name, k, 1)[:COLUMNS]
    label = '{} k={} kept tip rows'.format(name, k)
    got = []
    for tune in (None, dict(NO_KEEP_TIP_ROWS=1)):
        for eng in both(name, k, tune=tune):
            with eng:
                one_pass(eng, first)
                one_pass(eng, second)
                got.append(consume(eng, name))
    held(got[0], got[1], name, k, second, label)
    held(got[2], got[3], name, k, second, label + ' (NO_KEEP_TIP_ROWS)')
    assert_same(got[2], got[0], label)


@pytest.mark.parametrize('name, k', [('chained', 20), ('chained', 64)])
def test_a_sweep_of_a_column_subset(name, k):
    """A full pass, consumers; new parameters for columns 0, 2 and 3; a sweep of those columns and the top-down sweep; consumers
    over all columns.  The active columns have the reference's values at the new parameters, the idle ones -- their parameters
    did not change -- give word for word what they gave before.  (Every likelihood is positive: no refusal arises.)"""
    first, second = units.models(name, k, 0)[:COLUMNS], units.models(name, k, 1)[:COLUMNS]
    label = '{} k={} column subset'.format(name, k)
    active, idle = [0, 2, 3], [1, 4]
    got = []
    for eng in both(name, k):
        with eng:
            before_lnl = one_pass(eng, first)
            before = consume(eng, name)
            for c in active:
                eng.set_models([second[c]], col_begin=c)
            eng.bottom_up_submit(True, active=np.array([1, 0, 1, 1, 0], dtype=np.uint8))
            lnl = np.asarray(eng.bottom_up_collect(True))
            assert np.isfinite(lnl).all() and np.array_equal(lnl[idle], before_lnl[idle])
            assert not np.isin(lnl[active], before_lnl[active]).any()
            eng.top_down_marginals(posterior=False, lh=False)
            got.append((before, consume(eng, name)))
    held(got[0][0], got[1][0], name, k, first, label + ', full pass')
    held(got[0][1], got[1][1], name, k, mixed(first, second, active), label + ', after the subset')
    assert_same(got[0][1], got[0][0], label, cols=idle)


@pytest.mark.parametrize('name, k', ORDER_CASES)
def test_a_joint_pass_in_between(name, k):
    """joint_pass() between the marginal pass and a consumer: every consumer is refused by name; after a new marginal pass they
    answer with the reference's values."""
    models = units.models(name, k)[:COLUMNS]
    label = '{} k={} joint pass in between'.format(name, k)
    got = []
    for eng in both(name, k):
        with eng:
            one_pass(eng, models)
            assert np.isfinite(eng.joint_pass()[0]).all()
            for key in CONSUMERS:
                with pytest.raises(hip.HipError) as refused:
                    CONSUMERS[key](eng, name)
                assert refused.value.status == hip.PML_ERR_INVALID and NEED_PASS in str(refused.value), (key, str(refused.value))
            one_pass(eng, models)
            got.append(consume(eng, name))
    held(got[0], got[1], name, k, models, label)
