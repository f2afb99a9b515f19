"""
pml_history_through_time / Engine.history_through_time / ml.expected_history_through_time on the device against the exact
reference at 60 digits (tests/history_time_ref.py: the tree subdivided at the boundaries, whole-branch sums only), the identities
on the device's own output, bit-reproducibility over schedules, numberings, columns, calls and bins, and the refusals.

Error measure: that of test_gpu_expected_history.py.  Every term of every sum is non-negative, so it is the plain relative error
|device - exact| / exact per entry of times, jumps and lineages; where the exact value is 0 the device's has to be exactly 0.
The cap is that file's 1e-11 and its STORED_E_TOLERANCE = 1e-12, for its reasons: a float64 evaluation of the coefficients stays
below 2e-15, a dropped term or a wrong coefficient is 1e-3 or more; what lies between is the rounding of e_n = exp(-mu t'_n) to a
double in the marginal pass, which leaves 1 - e_n of a branch of 1e-12 off by 1e-4 of itself.  TOLERANCE = min(8 x the worst
ratio seen on an MI355X, 1e-11); the worst ratio is recorded in profiles/history_through_time.txt.  It is 1.35e-11 (jumps; lineages
1.27e-11, times 3.66e-12), in test_branches_of_1e_9_and_1e_12_cut_by_a_boundary at k = 65, so TOLERANCE is the cap itself; every
other case of the file stays below 1.6e-14.  A case above the cap passes only if the reference run on the exponentials the device
stored reproduces the gap and the device agrees with THAT to STORED_E_TOLERANCE: that one case does -- the stored exponentials
move the reference by the same 1.35e-11, and the device is within 1.3e-15 of it.

(The reference subdivides branches, which is the same model only where the frequencies sum to 1; the doubles the device gets sum
to 1 +- 1e-16, five digits below the tolerance.  test_history_time_ref.py holds the two routes of the reference to 1e-50.)
"""
import os

import numpy as np
import pandas as pd
import pytest

import expected_history_ref as href
import history_time_ref as tref
import loglik_gradient_cases as cases
from conftest import load_golden, GOLDEN
from pastml_amd import hip, ml
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.models.F81Model import F81Model
from pastml_amd.models.HKYModel import HKYModel
from pastml_amd.tree import FlatForest, annotate_dates, read_tree

pytestmark = pytest.mark.gpu

WORST_SEEN = 1.35e-11   # (jumps, test_branches_of_1e_9_and_1e_12_cut_by_a_boundary at k = 65; every other case: 1.6e-14)
TOLERANCE = min(8 * WORST_SEEN, 1e-11)
assert TOLERANCE <= 1e-11
STORED_E_TOLERANCE = 1e-12
IDENTITY = 1e-12

DATA = os.path.join(GOLDEN, 'data')
TREE_NWK = os.path.join(DATA, 'Albanian.tree.152tax.tre')
STATES_INPUT = os.path.join(DATA, 'data.txt')


def _model(kind, k, seed, tau):
    return dict(kind=hip.KIND_F81, pi=cases.frequencies(kind, k, seed)), cases.rates(seed, tau)


def _device(flat, masks_cols, models, k, t, bounds, tune=None, cols=None, calls=1, jumps=True, lineages=True, whole=False,
            stored_e=False):
    """(times, jumps, lineages) of Engine.history_through_time; with ``whole`` also Engine.expected_history's (times, jumps) of
    the same context, with ``stored_e`` the exponentials the marginal pass stored for column 0."""
    with hip.Engine(flat, len(models), k, tune=tune) as eng:
        eng.set_models(models)
        eng.set_masks(np.asarray(masks_cols))
        eng.marginal_pass(posterior=False, lh=False)
        for _ in range(calls):
            out = eng.history_through_time(t, bounds, *(cols or ()), jumps=jumps, lineages=lineages)
        if whole:
            out = out + (eng.expected_history(*(cols or ()))[:2],)
        if stored_e:
            out = out + (eng.download(hip.BUF_BRANCH_EXP, 0),)
        return out


def _jump_rows(k):
    return None if k <= 65 else [0, 15, 16, 63, 64, k - 17, k - 2, k - 1]


def _ratios(got, ref):
    """(times, jumps, lineages): the worst relative error of each against a reference dict."""
    times, jumps, lineages = got
    M = len(ref['times'])
    assert times.shape[0] == M and lineages.shape[0] == M + 1
    assert np.isfinite(times).all() and np.isfinite(jumps).all() and np.isfinite(lineages).all()
    r_times = max(href.relative_errors(times[m], ref['times'][m]).max() for m in range(M))
    r_lineages = max(href.relative_errors(lineages[m], ref['lineages'][m]).max() for m in range(M + 1))
    r_jumps = max(href.relative_errors(jumps[m][i], ref['jumps'][m][i]).max() for m in range(M) for i in sorted(ref['jumps'][m]))
    return r_times, r_jumps, r_lineages


def _check(got, flat, masks, model, t, bounds, label, rows='by k', route=tref.by_subdivision):
    """One column's (times [M, k], jumps [M, k, k], lineages [M + 1, k]) against the reference; the ratios are printed, then held."""
    spec, (sf, tau, tf) = model
    k = got[0].shape[1]
    rows = _jump_rows(k) if rows == 'by k' else rows
    ref = route(flat, masks, spec['pi'], t, bounds, sf, tau, tf, jump_rows=rows)
    for m in range(len(bounds) - 1):
        assert (np.diag(got[1][m]) == 0).all(), label
    r = _ratios(got, ref)
    print('ratio {}: times {:.3g} jumps {:.3g} lineages {:.3g}'.format(label, *r))
    assert max(r) <= TOLERANCE, (label,) + r
    return ref


KS = (2, 4, 5, 16, 17, 64, 65, 256, 257, 512)
CASES = [(kind, k) for kind in ('F81', 'JC') for k in KS]


@pytest.mark.parametrize('shape', cases.SHAPES)
@pytest.mark.parametrize('kind, k', CASES)
def test_device_against_the_reference(kind, k, shape):
    """Every shape at one k per lane shape of the segment pass and per tiling of the product, F81 and JC, tau = 0 and tau > 0:
    five bins that line up with no node but for one boundary put exactly on a node time; the roots of a forest begin at
    different times."""
    i = CASES.index((kind, k))
    flat = cases.forest(shape, seed=i % 3)
    masks = cases.masks(flat, k, i)
    t = tref.root_distance(flat, stagger=0.21)
    bounds = tref.covering_boundaries(t, 5)
    assert np.isin(bounds, t).sum() == 1
    for tau in (0.0, 0.011):
        model = _model(kind, k, i % 4, tau)
        label = '{} k={} {} tau={}'.format(kind, k, shape, tau)
        times, jumps, lineages = _device(flat, [masks], [model], k, t, bounds)
        _check((times[0], jumps[0], lineages[0]), flat, masks, model, t, bounds, label)


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [5, 65])
def test_empty_bins_and_a_tree_partly_outside(k):
    flat = cases.forest('forest')
    masks = cases.masks(flat, k, 3)
    model = _model('F81', k, 1, 0.011)
    t = tref.root_distance(flat, stagger=0.4)
    lo, hi = t.min(), t.max()
    span = hi - lo
    # two bins before the first root, the tree in three bins, two bins after the last tip
    bounds = np.array([lo - 3.0, lo - 2.0, lo - 1e-3, lo + 0.31 * span, lo + 0.62 * span, hi + 1e-3, hi + 1.0, hi + 2.0])
    times, jumps, lineages = _device(flat, [masks], [model], k, t, bounds)
    for m in (0, 1, 5, 6):
        assert (times[0][m] == 0).all() and (jumps[0][m] == 0).all(), m
    for m in (0, 1, 2, 5, 6, 7):
        assert (lineages[0][m] == 0).all(), m
    _check((times[0], jumps[0], lineages[0]), flat, masks, model, t, bounds, 'empty bins k={}'.format(k))
    part = np.array([lo + 0.27 * span, lo + 0.5 * span, lo + 0.71 * span])
    times, jumps, lineages = _device(flat, [masks], [model], k, t, part)
    _check((times[0], jumps[0], lineages[0]), flat, masks, model, t, part, 'partly outside k={}'.format(k))


@pytest.mark.parametrize('k', [4, 17])
def test_zero_extent_branches_with_smoothed_length(k):
    """tau > 0 gives a branch without extent a length; it is counted whole in the bin that contains it -- also where its time is
    a boundary, and the last one --, and not at all outside the bins."""
    flat = cases.forest('zeros')
    zero = np.flatnonzero((flat.parent >= 0) & (flat.dist == 0))
    assert len(zero) >= 3
    masks = cases.masks(flat, k, 7)
    model = _model('F81', k, 2, 0.02)
    t = tref.root_distance(flat, stagger=0.1)
    on = np.unique(t[zero])
    on = on[(on > t.min()) & (on < t.max())]
    assert len(on) >= 2
    for bounds in (np.array([t.min() - 0.5, on[0], on[-1], t.max() + 0.5]), np.array([t.min() - 0.5, on[0], on[-1]]),
                   np.array([on[0] + 1e-9, t.max() + 0.5])):
        times, jumps, lineages = _device(flat, [masks], [model], k, t, bounds)
        _check((times[0], jumps[0], lineages[0]), flat, masks, model, t, bounds, 'zero extents k={} M={}'.format(k, len(bounds) - 1))


@pytest.mark.parametrize('k', [5, 65])
def test_branches_of_1e_9_and_1e_12_cut_by_a_boundary(k):
    flat = cases.forest('ragged')
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[3::7]] = 1e-9
    flat.dist[branches[5::7]] = 1e-12
    masks = cases.masks(flat, k, 2)
    model = _model('F81', k, 1, 0.0)
    spec, (sf, tau, tf) = model
    t = tref.root_distance(flat)
    cut = [n for n in list(branches[3::7]) + list(branches[5::7]) if t[n] > t[flat.parent[n]]]
    mids = np.unique([0.5 * (t[n] + t[flat.parent[n]]) for n in cut])
    mids = mids[[0, len(mids) // 3, 2 * len(mids) // 3, len(mids) - 1]]
    bounds = np.unique(np.concatenate(([t.min() - 0.1], mids, [t.max() + 0.1])))
    n_cut = sum(int(((t[flat.parent[n]] < bounds) & (bounds < t[n])).any()) for n in cut)
    assert n_cut >= 3, n_cut
    times, jumps, lineages, e = _device(flat, [masks], [model], k, t, bounds, stored_e=True)
    got = (times[0], jumps[0], lineages[0])
    assert (e[flat.parent >= 0] < 1.0).all()
    exact = tref.by_subdivision(flat, masks, spec['pi'], t, bounds, sf, tau, tf)
    r = _ratios(got, exact)
    print('ratio near-zero branches k={}: times {:.3g} jumps {:.3g} lineages {:.3g}'.format(k, *r))
    # against the marginal pass restated on the exponentials the device stored: what is left is this pass's own arithmetic
    stored = tref.by_coefficients(flat, masks, spec['pi'], t, bounds, sf, tau, tf, stored_e=e)
    r_stored = _ratios(got, stored)
    print('ratio near-zero branches k={} on the stored exponentials: times {:.3g} jumps {:.3g} lineages {:.3g}'.format(k, *r_stored))
    assert max(r_stored) <= STORED_E_TOLERANCE, r_stored
    if max(r) > TOLERANCE:
        # above the cap only if the stored exponentials reproduce the gap
        M = len(bounds) - 1
        gap = max(max(href.relative_errors([float(x) for x in stored[name][m]], exact[name][m]).max()
                      for m in range(len(exact[name]))) for name in ('times', 'lineages'))
        gap = max(gap, max(href.relative_errors([float(x) for x in stored['jumps'][m][i]], exact['jumps'][m][i]).max()
                           for m in range(M) for i in range(k)))
        print('gap of the stored exponentials k={}: {:.3g}'.format(k, gap))
        assert abs(gap - max(r)) <= STORED_E_TOLERANCE, (r, gap)


@pytest.mark.parametrize('k', [5, 65])
def test_long_branches_cut_in_the_middle(k):
    """x = mu t' = 800: e_n underflows to 0 in the marginal pass; the two halves have exp(-400)."""
    flat = cases.forest('ragged')
    masks = cases.masks(flat, k, 4)
    model = _model('F81', k, 2, 0.0)
    spec, (sf, tau, tf) = model
    mu = 1.0 / (1.0 - spec['pi'].dot(spec['pi']))
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[::5]] = 800.0 / (mu * sf * tf)
    t = tref.root_distance(flat)
    mids = np.unique([0.5 * (t[n] + t[flat.parent[n]]) for n in branches[::5]])
    bounds = np.unique(np.concatenate(([t.min() - 1.0], mids[:: max(1, len(mids) // 4)], [t.max() + 1.0])))
    times, jumps, lineages, e = _device(flat, [masks], [model], k, t, bounds, stored_e=True)
    assert (e[branches[::5]] == 0.0).all()
    _check((times[0], jumps[0], lineages[0]), flat, masks, model, t, bounds, 'long branches k={}'.format(k))


def test_200_bins_on_a_3_tip_tree():
    k = 4
    flat = FlatForest.random(3, seed=1, max_arity=2, zero_frac=0.0, n_trees=1)
    masks = cases.masks(flat, k, 0)
    model = _model('F81', k, 0, 0.0)
    t = tref.root_distance(flat)
    bounds = np.linspace(t.min(), t.max(), 201)
    times, jumps, lineages = _device(flat, [masks], [model], k, t, bounds)
    _check((times[0], jumps[0], lineages[0]), flat, masks, model, t, bounds, '200 bins')


# ---------------------------------------------------------------------------------------------------------------------
# pieces
# ---------------------------------------------------------------------------------------------------------------------

# (k, segments per piece): the segment pass's 1024, 512 and 256 (history_piece), the jump product's 2048 and 4096
# (history_jump_piece; pml_launch_history.hip)
PIECES = [(4, 1024), (5, 512), (65, 256), (2, 2048), (65, 4096)]


def _two_bins(piece):
    """A forest and a boundary T1 such that exactly 2 piece + 37 branches begin before T1 -- the segments of the bin before it
    -- and more than one piece's worth reach beyond it."""
    want = 2 * piece + 37
    for seed in range(40):
        flat = FlatForest.random(piece + piece // 3 + 60, seed=seed, max_arity=3, zero_frac=0.0, n_trees=1)
        t = tref.root_distance(flat)
        has = flat.parent >= 0
        starts = np.sort(t[flat.parent[has]])
        if len(starts) > want and starts[want - 1] < starts[want]:
            T1 = 0.5 * (starts[want - 1] + starts[want])
            if not np.isin(T1, t):
                return flat, t, np.array([t.min() - 1.0, T1, t.max() + 1.0])
    raise AssertionError('no forest with a boundary after {} branch starts'.format(want))


@pytest.mark.parametrize('k, piece', PIECES)
def test_more_segments_than_one_piece_in_a_bin(k, piece):
    """One bin of 2 x piece + 37 segments, once per piece size of the launcher; the second bin begins in the middle of what
    would be a piece if the pieces were cut over the bins.  (The reference by its coefficient route, which test_history_time_ref
    holds to the subdivided tree at 1e-50: it keeps the forest at its size.)"""
    flat, t, bounds = _two_bins(piece)
    has = flat.parent >= 0
    assert int((t[flat.parent[has]] < bounds[1]).sum()) == 2 * piece + 37 and (2 * piece + 37) % piece != 0
    assert int((t[has] > bounds[1]).sum()) > 37
    masks = cases.masks(flat, k, 3)
    model = _model('F81', k, 2, 0.0)
    times, jumps, lineages = _device(flat, [masks], [model], k, t, bounds)
    rows = None if k * flat.n_nodes <= 70000 else [0, 15, k - 1]
    _check((times[0], jumps[0], lineages[0]), flat, masks, model, t, bounds, 'pieces k={} piece={}'.format(k, piece), rows=rows,
           route=tref.by_coefficients)


# ---------------------------------------------------------------------------------------------------------------------
# identities on the device's output alone
# ---------------------------------------------------------------------------------------------------------------------

def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool((np.abs(a - b) <= IDENTITY * np.abs(b)).all())


@pytest.mark.parametrize('shape', ['forest', 'zeros'])
@pytest.mark.parametrize('k', [4, 24, 130])
def test_identities(k, shape):
    flat = cases.forest(shape)
    masks = cases.masks(flat, k, 6)
    model = _model('F81', k, 3, 0.011)
    _, (sf, tau, tf) = model
    t = tref.root_distance(flat, stagger=0.3)
    length = np.where(flat.parent >= 0, (flat.dist + tau) * tf, 0.0)
    cover = tref.covering_boundaries(t, 7)
    part = cover[2:6]
    for bounds in (cover, part, cover[[0, -1]]):
        times, jumps, lineages, (whole_times, whole_jumps) = _device(flat, [masks], [model], k, t, bounds, whole=True)
        # the dwell times of a bin sum to the smoothed length inside it
        bin_length = ml.time_bin_fractions(flat, t, bounds).dot(length)
        assert _close(times[0].sum(axis=1), bin_length), (k, shape, len(bounds))
        # a lineage row sums to the number of branches alive at its boundary
        count = tref.crossing(flat.parent, t, bounds)
        assert count.max() > 0 or len(bounds) == 2
        assert (np.abs(lineages[0].sum(axis=1) - count) <= IDENTITY * np.maximum(count, 1)).all(), (k, shape, len(bounds))
        assert (lineages[0][count == 0] == 0).all()
        if bounds is not part:
            # bins that cover the tree -- one bin too -- sum to expected_history of the same context
            assert abs(bin_length.sum() - length.sum()) <= IDENTITY * length.sum()
            assert _close(times[0].sum(axis=0), whole_times[0]), (k, shape, len(bounds))
            assert _close(jumps[0].sum(axis=0), whole_jumps[0]), (k, shape, len(bounds))


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('k, n_tips', [(4, 3000), (24, 1500), (130, 700)])
def test_bits_do_not_depend_on_schedules_numbering_column_or_call(k, n_tips):
    flat = FlatForest.random(n_tips, seed=11, max_arity=3, zero_frac=0.0, n_trees=2)
    masks = cases.masks(flat, k, 1)
    model = _model('F81', k, 1, 0.0)
    t = tref.root_distance(flat, stagger=0.05)
    bounds = tref.covering_boundaries(t, 6)
    args = (k, t, bounds)
    base = _device(flat, [masks], [model], *args)
    assert all(np.isfinite(x).all() for x in base)
    assert _same(base, _device(flat, [masks], [model], *args, calls=2))
    assert _same(base, _device(flat, [masks], [model], *args, tune={'NO_SUPER': 1}))
    assert _same(base, _device(flat, [masks], [model], *args, tune={'NO_HEIGHT_ORDER': 1}))   # (the caller's numbering kept)
    others = [cases.masks(flat, k, 50 + c) for c in range(6)]
    other_models = [_model('F81', k, c % 4, 0.01 * (c % 2)) for c in range(6)]
    first = _device(flat, [masks] + others, [model] + other_models, *args)
    last = _device(flat, others + [masks], other_models + [model], *args)
    assert _same([x[0] for x in first], [x[0] for x in base])
    assert _same([x[6] for x in last], [x[0] for x in base])
    assert _same([x[1:] for x in first], [x[:6] for x in last])
    # a sub-range of the columns is the same columns
    sub = _device(flat, [masks] + others, [model] + other_models, *args, cols=(2, 5))
    assert _same(sub, [x[2:5] for x in first])


@pytest.mark.parametrize('k', [4, 24, 130])
def test_times_have_the_same_bits_whatever_else_is_asked_for(k):
    flat = cases.forest('polytomy')
    masks = cases.masks(flat, k, 5)
    model = _model('F81', k, 3, 0.011)
    t = tref.root_distance(flat)
    bounds = tref.covering_boundaries(t, 4)
    full = _device(flat, [masks], [model], k, t, bounds)
    for jumps, lineages in ((False, False), (True, False), (False, True)):
        got = _device(flat, [masks], [model], k, t, bounds, jumps=jumps, lineages=lineages)
        assert np.array_equal(got[0], full[0])
        assert (got[1] is None) == (not jumps) and (got[2] is None) == (not lineages)
        assert got[1] is None or np.array_equal(got[1], full[1])
        assert got[2] is None or np.array_equal(got[2], full[2])


@pytest.mark.parametrize('k', [5, 70])
def test_a_bins_row_does_not_change_when_bins_are_appended(k):
    flat = FlatForest.random(900, seed=4, max_arity=3, zero_frac=0.0, n_trees=2)
    masks = cases.masks(flat, k, 8)
    model = _model('F81', k, 0, 0.0)
    t = tref.root_distance(flat, stagger=0.2)
    bounds = tref.covering_boundaries(t, 9)
    long_call = _device(flat, [masks], [model], k, t, bounds)
    short_call = _device(flat, [masks], [model], k, t, bounds[:5])
    assert np.array_equal(short_call[0], long_call[0][:, :4]) and np.array_equal(short_call[1], long_call[1][:, :4])
    assert np.array_equal(short_call[2][:, :4], long_call[2][:, :4])   # (the boundaries that begin a bin in both calls)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------

def _refused(eng, t, bounds, status, *words):
    with pytest.raises(hip.HipError) as info:
        eng.history_through_time(t, bounds)
    assert info.value.status == status, str(info.value)
    for word in words:
        assert word in str(info.value), str(info.value)


def test_refusals_leave_the_context_answering():
    flat = cases.forest('balanced')
    t = tref.root_distance(flat)
    bounds = tref.covering_boundaries(t, 3)
    # no marginal pass
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([_model('F81', 4, 0, 0.0)])
        eng.set_masks(np.asarray([cases.masks(flat, 4, 0)]))
        _refused(eng, t, bounds, hip.PML_ERR_INVALID, 'pml_history_through_time', 'marginal')
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts()
        first = eng.history_through_time(t, bounds)
        assert all(np.isfinite(x).all() for x in first)
        # descending boundaries, M = 0, a child before its parent, a time that is not a number
        _refused(eng, t, bounds[::-1], hip.PML_ERR_INVALID, 'pml_history_through_time', 'ascending')
        _refused(eng, t, bounds[:1], hip.PML_ERR_INVALID, 'M = 0')
        early = t.copy()
        early[17] = early[flat.parent[17]] - 0.5
        _refused(eng, early, bounds, hip.PML_ERR_INVALID, 'node 17 is earlier than its parent {}'.format(flat.parent[17]))
        early[17] = np.nan
        _refused(eng, early, bounds, hip.PML_ERR_INVALID, 'node 17', 'finite')
        # too many bins for the scratch of one call
        many = np.linspace(t.min(), t.max(), (1 << 24) // 16 + 2)
        _refused(eng, t, many, hip.PML_ERR_UNSUPPORTED, 'PML_HIST_TIME_MAX_CELLS')
        assert np.array_equal(eng.expected_counts(), counts)   # (the results of the pass stay)
        assert _same(first, eng.history_through_time(t, bounds))
    # a model kind other than F81
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([(dict(kind=hip.KIND_HKY, pi=cases.frequencies('F81', 4, 0), kappa=2.0), cases.rates(0, 0.0))])
        eng.set_masks(np.asarray([cases.masks(flat, 4, 0)]))
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, t, bounds, hip.PML_ERR_UNSUPPORTED, 'F81', 'HKY')
        assert np.isfinite(eng.expected_counts()).all()
    # a column whose pi . pi is 1, one state
    with hip.Engine(flat, 2, 2) as eng:
        eng.set_models([_model('F81', 2, 0, 0.0), (dict(kind=hip.KIND_F81, pi=np.array([1.0, 0.0])), cases.rates(0, 0.0))])
        masks = np.ones((2, flat.n_nodes, 2), dtype=np.int8)
        masks[:, flat.tips[::2], 1] = 0
        eng.set_masks(masks)
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, t, bounds, hip.PML_ERR_INVALID, 'column 1', 'pi . pi')
        assert np.isfinite(eng.history_through_time(t, bounds, 0, 1)[0]).all()   # (the other column is served)
    with hip.Engine(flat, 1, 1) as eng:
        eng.set_models([(dict(kind=hip.KIND_F81, pi=np.array([1.0])), cases.rates(0, 0.0))])
        eng.set_masks(np.ones((1, flat.n_nodes, 1), dtype=np.int8))
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, t, bounds, hip.PML_ERR_INVALID, 'k = 1')
        assert np.isfinite(eng.expected_counts()).all()


def test_front_end_refuses_other_models_by_name():
    flat = cases.forest('balanced')
    roots = flat.to_tree_nodes()
    model = HKYModel(forest_stats=ForestStats(roots), sf=1.0)
    with pytest.raises(NotImplementedError, match='HKY') as info:
        ml.expected_history_through_time(roots, 'c', model, 4)
    assert 'PML_ERR_UNSUPPORTED' in str(info.value) and 'expected_history_through_time' in str(info.value)


# ---------------------------------------------------------------------------------------------------------------------
# the front end on the Albania tree
# ---------------------------------------------------------------------------------------------------------------------

def test_front_end_on_the_albania_tree():
    zz = load_golden('albania_F81')
    tree = read_tree(TREE_NWK)
    preannotate_forest([tree], df=pd.read_csv(STATES_INPUT, index_col=0, header=0)[['Country']])
    stats = ForestStats([tree])
    f81 = F81Model(states=zz['opt_states'], forest_stats=stats, sf=float(zz['opt_sf']), frequencies=zz['opt_frequencies'])
    k = len(f81.states)
    before = ml.loglikelihood_gradient([tree], 'Country', f81)['log_likelihood']
    whole = ml.expected_history([tree], 'Country', f81)
    out = ml.expected_history_through_time([tree], 'Country', f81, 6)
    assert sorted(out) == ['bin_length', 'boundaries', 'jumps', 'lineages', 'log_likelihood', 'states', 'times', 'tree_length']
    assert out['times'].shape == (6, k) and out['jumps'].shape == (6, k, k) and out['lineages'].shape == (7, k)
    assert out['boundaries'].shape == (7,) and out['bin_length'].shape == (6,) and list(out['states']) == list(f81.states)
    assert out['log_likelihood'] == whole['log_likelihood'] == before
    # the masks are restored: the same forest gives the ln L it gave before
    assert ml.loglikelihood_gradient([tree], 'Country', f81)['log_likelihood'] == before
    # six equal bins from the root to the latest tip hold the whole tree
    assert abs(out['bin_length'].sum() - out['tree_length']) <= IDENTITY * out['tree_length']
    assert _close(out['times'].sum(axis=1), out['bin_length'])
    assert _close(out['times'].sum(axis=0), whole['times'])
    assert _close(out['jumps'].sum(axis=0), whole['jumps'])
    flat = ml.get_flat_forest([tree])
    dates = annotate_dates(flat)
    assert out['boundaries'][0] == dates.min() and out['boundaries'][-1] == dates[flat.tips].max()
    count = tref.crossing(flat.parent, dates, out['boundaries'])
    assert (np.abs(out['lineages'].sum(axis=1) - count) <= IDENTITY * np.maximum(count, 1)).all()
    # given boundaries and root dates shift everything; jumps left out
    shifted = ml.expected_history_through_time([tree], 'Country', f81, out['boundaries'] + 1990.0, root_dates=[1990.0], jumps=False)
    assert shifted['jumps'] is None
    assert np.abs(shifted['times'] - out['times']).max() <= 1e-9 * out['times'].max()
