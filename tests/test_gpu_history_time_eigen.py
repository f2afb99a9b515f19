"""
pml_history_through_time_eigen / Engine.history_through_time_eigen / ml.expected_history_through_time_general on the device against
the 60-digit restatement of the header's sums (tests/history_time_eigen_ref.by_scaling, which tests/test_history_time_eigen_ref.py
holds to the subdivided tree at 1e-55), the identities on the device's own output, bit-reproducibility over calls, columns, what
is asked for and bins, and the refusals.

Error measure: test_gpu_expected_history_eigen.py's -- |device - exact| / (the largest |entry| of the exact array), per output
and PER BIN (times [k], the jump rows held, lineages [k] of one bin or boundary): the sums have mixed signs.  TOLERANCE is 8 x the
worst ratio seen on an MI355X over all the cases of this file (room for another box's summation order), recorded in
profiles/history_through_time_eigen.txt, and must not exceed 1e-9: a dropped term or a wrong coefficient shows at 1e-3 or more.
The worst ratio seen is 2.84e-12 (lineages; jumps 2.77e-12, times 1.67e-13), in test_branches_of_1e_9_and_1e_12_cut_by_a_boundary
at k = 61 -- the case that gives the whole-tree entry its worst, 2.21e-12 --; next come the same tree at k = 5 (7.05e-13), the
nine-tip tree at k = 65 (4.24e-13), an F81 model as an eigen model at k = 65 against the F81 entry (3.09e-13) and the nine-tip
tree at k = 128 (2.17e-13).  Every other case stays under 1e-13.  8 x 2.84e-12 = 2.27e-11 is under the 1e-9 cap.

The identities, in float64 on what the device returned, to TOLERANCE of the gross of their two sides: a row of times sums to the
smoothed length in its bin; the bins of a call that covers the tree sum to pml_expected_history_eigen on the same context; a
lineage row sums to the number of branches alive; an F81 model handed over as an eigen model agrees with pml_history_through_time
on an F81 context.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest

import expected_history_eigen_ref as eref
import history_time_eigen_cases as tcases
import history_time_eigen_ref as teref
import history_time_ref as tref
import loglik_gradient_cases as cases
from pastml_amd import hip, ml
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.models.F81Model import F81Model
from pastml_amd.models.HKYModel import HKYModel
from pastml_amd.models.JTTModel import JTTModel, JTT_STATES
from pastml_amd.tree import annotate_dates, read_tree
from test_gpu_history_time import _two_bins
from test_gpu_parity import random_spec

pytestmark = pytest.mark.gpu

WORST_SEEN = 2.84e-12   # near-zero branches k=61, lineages (profiles/history_through_time_eigen.txt)
TOLERANCE = 8 * WORST_SEEN
assert TOLERANCE <= 1e-9

PIECE = 512   # PML_HEIG_PIECE
TILE = 16     # PML_HTE_TILE


def _device(flat, masks_cols, models, k, t, bounds, tune=None, cols=None, calls=1, jumps=True, lineages=True, whole=False):
    """(times, jumps, lineages) of Engine.history_through_time_eigen; with ``whole`` also Engine.expected_history_eigen's (times,
    jumps) of the same context."""
    with hip.Engine(flat, len(models), k, tune=tune) as eng:
        eng.set_models(models)
        eng.set_masks(np.asarray(masks_cols))
        eng.marginal_pass(posterior=False, lh=False)
        for _ in range(calls):
            out = eng.history_through_time_eigen(t, bounds, *(cols or ()), jumps=jumps, lineages=lineages)
        if whole:
            out = out + (eng.expected_history_eigen(*(cols or ()))[:2],)
        return out


def _jump_rows(k):
    return None if k < 65 else [0, 15, 16, 63, 64, k - 2, k - 1]


def _ratios(got, ref):
    """(times, jumps, lineages): the worst scaled error of each against a reference dict, bin by bin."""
    times, jumps, lineages = got
    M = len(ref['times'])
    assert times.shape[0] == M and jumps.shape[0] == M and lineages.shape[0] == M + 1
    r_times = max(eref.scaled_errors(times[m], ref['times'][m]).max() for m in range(M))
    r_lineages = max(eref.scaled_errors(lineages[m], ref['lineages'][m]).max() for m in range(M + 1))
    r_jumps = 0.0
    for m in range(M):
        rows = sorted(ref['jumps'][m])
        r_jumps = max(r_jumps, eref.scaled_errors(np.concatenate([jumps[m][i] for i in rows]),
                                                  [x for i in rows for x in ref['jumps'][m][i]]).max())
    return r_times, r_jumps, r_lineages


def _check(got, flat, masks, model, t, bounds, label, rows='by k'):
    """One column's (times [M, k], jumps [M, k, k], lineages [M + 1, k]) against the restatement; the ratios are printed, then
    held."""
    spec, (sf, tau, tf) = model
    k = got[0].shape[1]
    rows = _jump_rows(k) if rows == 'by k' else rows
    ref = teref.by_scaling(flat, masks, spec, t, bounds, sf, tau, tf, jump_rows=rows)
    for x in got:
        assert np.isfinite(x).all() and (x >= 0).all(), label
    for m in range(len(bounds) - 1):
        assert (np.diag(got[1][m]) == 0).all(), label
    r = _ratios(got, ref)
    print('ratio {}: times {:.3g} jumps {:.3g} lineages {:.3g}'.format(label, *r))
    assert max(r) <= TOLERANCE, (label,) + r
    return ref


def _check_identities(got, flat, model, t, bounds, label, whole=None):
    _, (sf, tau, tf) = model
    times, jumps, lineages = got
    length = np.where(flat.parent >= 0, (flat.dist + tau) * tf, 0.0)
    bin_length = ml.time_bin_fractions(flat, t, bounds).dot(length)
    assert (np.abs(times.sum(axis=1) - bin_length) <= TOLERANCE * bin_length).all(), (label, 'bin_length')
    count = tref.crossing(flat.parent, t, bounds)
    assert (np.abs(lineages.sum(axis=1) - count) <= TOLERANCE * np.maximum(count, 1)).all(), (label, 'lineages')
    assert (lineages[count == 0] == 0).all(), label
    if whole is not None:
        assert abs(bin_length.sum() - length.sum()) <= 1e-14 * length.sum(), label   # (the call covers the tree)
        for mine, theirs in zip((times, jumps), whole):
            gross = np.abs(mine).sum(axis=0) + np.abs(theirs)
            assert (np.abs(mine.sum(axis=0) - theirs) <= TOLERANCE * gross.max()).all(), (label, 'whole')


def _hky(kappa=3.0, forest_stats=None, sf=1.3):
    return HKYModel(forest_stats=forest_stats, sf=sf, frequencies=np.array([0.1, 0.35, 0.05, 0.5]), kappa=kappa)


def _spec(k, seed=0):
    if k == 4:
        return _hky().eigen_spec()
    if k == 20:
        return tcases.jtt_spec()
    return random_spec('EIGEN', k, np.random.default_rng(7000 + 3 * k + seed))


RATES = [(1.3, 0.0, 1.0), (0.8, 0.011, 0.95)]
KS = (2, 4, 15, 16, 17, 20, 33, 61, 65, 128)


@pytest.mark.parametrize('k', KS)
def test_device_against_the_reference(k):
    """The nine-tip tree -- polytomy, a branch with t' = 0 and an extent, a branch with length and no extent -- at every k of the
    lineage kernel's and the pair kernel's shapes: two columns, tau = 0 and tau > 0, with their own masks.  M = 7 up to 33 states
    (bins before and after the tree, a boundary on a node's time, slivers of 1e-12 of a branch next to its parent and next to its
    child), M = 3 beyond (part of the tree; the reference's products cost k^3 per bin); the library's numbering on, and off at
    three of them.  The identities on a call that covers the tree, at every k."""
    flat, t, ids = tcases.nine_tips()
    masks = [tcases.masks(flat, k, k), tcases.masks(flat, k, k + 1)]
    models = [(_spec(k), RATES[0]), (_spec(k, 1), RATES[1])]
    cover = tcases.boundaries(flat, t, ids, 7)
    bounds = cover if k <= 33 else tcases.boundaries(flat, t, ids, 3)
    for tune in (None, {'NO_HEIGHT_ORDER': 1}) if k in (4, 20, 65) else (None,):
        times, jumps, lineages = _device(flat, masks, models, k, t, bounds, tune=tune)
        for c in range(2):
            label = 'nine tips k={} M={} column {}{}'.format(k, len(bounds) - 1, c, ' caller numbering' if tune else '')
            got = (times[c], jumps[c], lineages[c])
            _check(got, flat, masks[c], models[c], t, bounds, label)
            _check_identities(got, flat, models[c], t, bounds, label)
            if len(bounds) == 8:   # empty bins and boundaries outside the tree: exact zeros
                assert (times[c][[0, 6]] == 0).all() and (jumps[c][[0, 6]] == 0).all() and (lineages[c][[0, 1, 6, 7]] == 0).all()
    times, jumps, lineages, whole = _device(flat, masks, models, k, t, cover, whole=True)
    for c in range(2):
        _check_identities((times[c], jumps[c], lineages[c]), flat, models[c], t, cover, 'nine tips cover k={}'.format(k),
                          whole=(whole[0][c], whole[1][c]))


def _two_binary_sites(a):
    """A CUSTOM_RATES-like model of 4 states by hand, every double exact: two independent binary sites that flip at rate a / 2
    each.  Eigenvalues 0, -a, -a, -2a: two exactly equal."""
    one = np.array([[1.0, 1.0], [1.0, -1.0]])
    A = np.kron(one, one)
    return dict(kind=hip.KIND_EIGEN, pi=np.full(4, 0.25), d=np.array([0.0, -a, -a, -2 * a]), A=A, Ainv=A / 4.0)


def test_equal_eigenvalues_and_both_sides_of_the_switch_within_one_branch():
    """The branch above t7 has t' = 0.6 and is cut at a quarter: the pairs with |d_c - d_d| = 2 have |z| = 0.3 in its first
    segment (the series) and 0.9 in its second (the quotient); the pair of equal eigenvalues takes the series at z = 0."""
    flat, t, ids = tcases.nine_tips()
    spec, rates = _two_binary_sites(2.0), (1.5, 0.0, 1.0)
    n = ids['t7']
    p = int(flat.parent[n])
    bounds = np.array([t.min() - 0.1, t[p] + 0.25 * (t[n] - t[p]), t.max() + 0.1])
    z = 2.0 * flat.dist[n] * 1.5 * np.array([0.25, 0.75])
    assert z[0] < eref.SWITCH < z[1] and spec['d'][1] == spec['d'][2]
    masks = tcases.masks(flat, 4, 9)
    times, jumps, lineages, whole = _device(flat, [masks], [(spec, rates)], 4, t, bounds, whole=True)
    got = (times[0], jumps[0], lineages[0])
    _check(got, flat, masks, (spec, rates), t, bounds, 'two binary sites')
    _check_identities(got, flat, (spec, rates), t, bounds, 'two binary sites', whole=(whole[0][0], whole[1][0]))


# ---------------------------------------------------------------------------------------------------------------------
# pieces and tiles
# ---------------------------------------------------------------------------------------------------------------------

def test_more_segments_than_one_piece_in_a_bin():
    """k = 4: one bin of 2 x 512 + 37 segments; the second bin begins in the middle of what would be a piece if the pieces were
    cut over the bins."""
    flat, t, bounds = _two_bins(PIECE)
    has = flat.parent >= 0
    assert int((t[flat.parent[has]] < bounds[1]).sum()) == 2 * PIECE + 37
    masks = cases.masks(flat, 4, 3)
    model = (_spec(4), (1.1, 0.0, 1.0))
    times, jumps, lineages = _device(flat, [masks], [model], 4, t, bounds)
    got = (times[0], jumps[0], lineages[0])
    _check(got, flat, masks, model, t, bounds, 'pieces k=4')
    _check_identities(got, flat, model, t, bounds, 'pieces k=4')


@pytest.mark.parametrize('k', [4, 20])
def test_flagged_segments_that_do_not_fill_their_last_tile(k):
    """More than 16 and not a multiple of 16 branches alive at a boundary, below and from 16 states on."""
    flat = cases.forest('forest')
    t = tref.root_distance(flat)
    inner = np.unique(t)
    mids = 0.5 * (inner[1:] + inner[:-1])
    alive = tref.crossing(flat.parent, t, mids)
    most = int(np.argmax(alive))
    assert alive[most] > TILE and alive[most] % TILE > 1
    bounds = np.array([t.min() - 0.1, mids[most], t.max() + 0.1])
    masks = cases.masks(flat, k, 2)
    model = (_spec(k), RATES[1])
    times, jumps, lineages = _device(flat, [masks], [model], k, t, bounds)
    got = (times[0], jumps[0], lineages[0])
    _check(got, flat, masks, model, t, bounds, 'lineage tile tail k={} alive={}'.format(k, alive[most]))
    _check_identities(got, flat, model, t, bounds, 'lineage tile tail k={}'.format(k))


@pytest.mark.parametrize('k', [5, 61])
def test_branches_of_1e_9_and_1e_12_cut_by_a_boundary(k):
    flat = cases.forest('ragged')
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[3::7]] = 1e-9
    flat.dist[branches[5::7]] = 1e-12
    t = tref.root_distance(flat)
    cut = [n for n in list(branches[3::7]) + list(branches[5::7]) if t[n] > t[flat.parent[n]]]
    mids = np.unique([0.5 * (t[n] + t[flat.parent[n]]) for n in cut])
    mids = mids[[0, len(mids) // 2, len(mids) - 1]]
    bounds = np.unique(np.concatenate(([t.min() - 0.1], mids, [t.max() + 0.1])))
    assert sum(int(((t[flat.parent[n]] < bounds) & (bounds < t[n])).any()) for n in cut) >= 3
    masks = cases.masks(flat, k, 2)
    model = (_spec(k), (1.7, 0.0, 1.0))
    times, jumps, lineages = _device(flat, [masks], [model], k, t, bounds)
    got = (times[0], jumps[0], lineages[0])
    _check(got, flat, masks, model, t, bounds, 'near-zero branches k={}'.format(k))
    _check_identities(got, flat, model, t, bounds, 'near-zero branches k={}'.format(k))


# ---------------------------------------------------------------------------------------------------------------------
# the F81 family's entry
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [4, 65])
def test_f81_model_as_eigen_model_agrees_with_the_f81_entry(k):
    """Every non-zero eigenvalue equal; the two paths share no code."""
    flat = cases.forest('forest')
    masks = cases.masks(flat, k, 4)
    pi = cases.frequencies('F81', k, 1)
    rates = cases.rates(1, 0.011)
    t = tref.root_distance(flat, stagger=0.3)
    bounds = tref.covering_boundaries(t, 5)
    got = _device(flat, [masks], [(eref.f81_as_eigen(pi), rates)], k, t, bounds)
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([(dict(kind=hip.KIND_F81, pi=pi), rates)])
        eng.set_masks(np.asarray([masks]))
        eng.marginal_pass(posterior=False, lh=False)
        f81 = eng.history_through_time(t, bounds)
    r = []
    for x, y in zip(f81, got):
        rows = [m for m in range(x.shape[1]) if x[0][m].any()]
        assert all((y[0][m] == 0).all() for m in range(x.shape[1]) if m not in rows)
        r.append(max(np.abs(x[0][m] - y[0][m]).max() / np.abs(x[0][m]).max() for m in rows))
    print('ratio F81 as eigen k={} against the F81 entry: times {:.3g} jumps {:.3g} lineages {:.3g}'.format(k, *r))
    assert max(r) <= TOLERANCE, r


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _random_models(k, n, seed):
    rng = np.random.default_rng(seed)
    return [(random_spec('EIGEN', k, rng), (float(rng.uniform(0.5, 3)), 0.01 * (c % 2), 1.0 - 0.05 * (c % 2))) for c in range(n)]


@pytest.mark.parametrize('k', [4, 20, 70])
def test_bits_do_not_depend_on_call_column_outputs_or_other_bins(k):
    flat = cases.forest('forest')
    t = tref.root_distance(flat, stagger=0.2)
    bounds = tref.covering_boundaries(t, 3)
    masks = [cases.masks(flat, k, 50 + c) for c in range(3)]
    models = _random_models(k, 3, 170 + k)
    args = (k, t, bounds)
    base = _device(flat, masks[1:2], models[1:2], *args)
    assert all(np.isfinite(x).all() for x in base)
    # the same call twice; the column as the second of three; a sub-range of the columns
    assert _same(base, _device(flat, masks[1:2], models[1:2], *args, calls=2))
    three = _device(flat, masks, models, *args)
    assert _same(base, [x[1:2] for x in three])
    assert _same(base, _device(flat, masks, models, *args, cols=(1, 2)))
    # what is asked for
    for jumps, lineages in ((False, False), (True, False), (False, True)):
        got = _device(flat, masks[1:2], models[1:2], *args, jumps=jumps, lineages=lineages)
        assert np.array_equal(got[0], base[0])
        assert (got[1] is None) == (not jumps) and (got[2] is None) == (not lineages)
        assert got[1] is None or np.array_equal(got[1], base[1])
        assert got[2] is None or np.array_equal(got[2], base[2])
    # a bin alone
    for m in range(3):
        alone = _device(flat, masks[1:2], models[1:2], k, t, bounds[m:m + 2])
        assert np.array_equal(alone[0][:, 0], base[0][:, m]) and np.array_equal(alone[1][:, 0], base[1][:, m]), m
        assert np.array_equal(alone[2], base[2][:, m:m + 2]), m


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------

NAME = 'pml_history_through_time_eigen'
INVALID, UNSUPPORTED = hip.PML_ERR_INVALID, hip.PML_ERR_UNSUPPORTED
NO_PASS = (INVALID, NAME + ' needs a marginal pml_bottom_up and pml_top_down_marginals first')
NOT_EIGEN = (UNSUPPORTED, NAME + " is for the eigen-decomposed models: this context's model kind is F81 (F81, JC, EFT), which "
                                 "pml_history_through_time serves")
# the row of tests/test_gpu_reader_refusals.py's table for this entry (_range_row(NAME, 'eigen') with its own NOT_EIGEN): the range
# is checked right behind the model, the kind ahead of the pass
ROW = {'no model': (INVALID, 'model parameters of column 0 were never set'), 'no pass': NO_PASS, 'bottom-up only': NO_PASS,
       'bad column': (INVALID, 'column range [0, 3) out of 0..2'), 'no pass + bad column': (INVALID, 'column range [0, 3) out of 0..2'),
       'wrong kind': NOT_EIGEN, 'wrong kind + no pass': NOT_EIGEN}


def test_the_row_of_the_readers_table():
    """The states of tests/test_gpu_reader_refusals.py, the entry's home an eigen context.  Every refused call returns before its
    first launch."""
    from pastml_amd import synthetic
    K, C = 4, 2
    flat = synthetic.balanced_forest(3)
    rng = np.random.default_rng(3)
    masks = np.stack([synthetic.one_hot_masks(flat, K, synthetic.tip_states(len(flat.tips), K, c)) for c in range(C)])
    models = {'f81': [(random_spec('F81', K, rng), (1.1, 0.0, 1.0)) for _ in range(C)],
              'eigen': [(random_spec('EIGEN', K, rng), (1.3, 0.0, 1.0)) for _ in range(C)]}
    out = [np.zeros(4096) for _ in range(3)]
    node_time, bounds = np.zeros(flat.n_nodes), np.array([0.0, 1.0])

    def call(eng, ce=C):
        p = [x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for x in [node_time, bounds] + out]
        status = eng._lib.pml_history_through_time_eigen(eng._ctx, 0, ce, p[0], p[1], 1, p[2], p[3], p[4])
        return status, eng._lib.pml_last_error().decode() if status != hip.PML_OK else ''

    seen = {}
    with hip.Engine(flat, C, K) as f81, hip.Engine(flat, C, K) as eigen:
        seen['no model'] = call(eigen)
        for kind, eng in (('f81', f81), ('eigen', eigen)):
            eng.set_models(models[kind])
            eng.set_masks(masks)
        seen['no pass'] = call(eigen)
        seen['no pass + bad column'] = call(eigen, ce=C + 1)
        seen['wrong kind + no pass'] = call(f81)
        eigen.bottom_up(is_marginal=True)
        seen['bottom-up only'] = call(eigen)
        for eng in (f81, eigen):
            eng.marginal_pass(posterior=False, lh=False)
        seen['bad column'] = call(eigen, ce=C + 1)
        seen['wrong kind'] = call(f81)
        assert call(eigen) == (hip.PML_OK, '')
        for eng in (f81, eigen):
            assert np.isfinite(eng.expected_counts()).all()
    for column, cell in ROW.items():
        print('{:36s} {:24s} {}'.format(NAME, column, seen[column]))
    assert seen == ROW


def _refused(eng, t, bounds, status, *words, **kwargs):
    with pytest.raises(hip.HipError) as info:
        eng.history_through_time_eigen(t, bounds, *kwargs.get('cols', ()))
    assert info.value.status == status, str(info.value)
    for word in words:
        assert word in str(info.value), str(info.value)


def test_refusals_leave_the_context_answering():
    flat = cases.forest('balanced')
    t = tref.root_distance(flat)
    bounds = tref.covering_boundaries(t, 3)
    masks = np.asarray([cases.masks(flat, 4, 0)])
    eigen = _random_models(4, 2, 5)
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models(eigen[:1])
        eng.set_masks(masks)
        _refused(eng, t, bounds, INVALID, NAME, 'marginal')
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts()
        first = eng.history_through_time_eigen(t, bounds)
        assert all(np.isfinite(x).all() for x in first)
        # the plan's refusals, with the plan's messages
        _refused(eng, t, bounds[::-1], INVALID, NAME, 'boundary 1 is not above boundary 0: the boundaries must be strictly ascending')
        _refused(eng, t, bounds[:1], INVALID, 'M = 0: at least one time bin (two boundaries) is needed')
        early = t.copy()
        early[17] = early[flat.parent[17]] - 0.5
        _refused(eng, early, bounds, INVALID, 'node 17 is earlier than its parent {}'.format(flat.parent[17]))
        early[17] = np.nan
        _refused(eng, early, bounds, INVALID, 'the time of node 17 is not finite')
        infinite = bounds.copy()
        infinite[2] = np.inf
        _refused(eng, t, infinite, INVALID, 'boundary 2 is not finite')
        # too many bins for the scratch of one call
        many = np.linspace(t.min(), t.max(), (1 << 24) // 16 + 2)
        _refused(eng, t, many, UNSUPPORTED, 'M k^2 = 16777232 is beyond 16777216 (PML_HIST_TIME_MAX_CELLS)')
        assert np.array_equal(eng.expected_counts(), counts)   # (the results of the pass stay)
        assert _same(first, eng.history_through_time_eigen(t, bounds))
    # an F81 context is pointed to its own entry, an HKY context to the eigen form of the model
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([(dict(kind=hip.KIND_F81, pi=cases.frequencies('F81', 4, 0)), cases.rates(0, 0.0))])
        eng.set_masks(masks)
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts()
        _refused(eng, t, bounds, UNSUPPORTED, 'F81', 'which pml_history_through_time serves')
        assert np.array_equal(eng.expected_counts(), counts)
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([(dict(kind=hip.KIND_HKY, pi=cases.frequencies('F81', 4, 0), kappa=2.0), cases.rates(0, 0.0))])
        eng.set_masks(masks)
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts()
        _refused(eng, t, bounds, UNSUPPORTED, 'HKY', 'hand the model over as an eigen model')
        assert np.array_equal(eng.expected_counts(), counts)
    # a column whose eigenvalues are not finite: the message names the column, and a sub-range call serves the other one.  (A
    # scaling factor that is not finite and positive never gets as far as this entry: pml_model_set_eigen refuses it; nor do
    # more than 256 states: the sweeps of the matrix models hold no more, so no marginal pass comes first.)
    spec, rates = eigen[1]
    bad = (dict(spec, d=np.where(np.arange(4) == 2, -np.inf, spec['d'])), rates)
    with hip.Engine(flat, 2, 4) as eng:
        eng.set_models([eigen[0], eigen[0]])
        eng.set_masks(np.concatenate([masks, masks]))
        eng.marginal_pass(posterior=False, lh=False)
        good = eng.history_through_time_eigen(t, bounds, 0, 1)
        eng.set_models([bad], col_begin=1)
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts(0, 1)
        _refused(eng, t, bounds, INVALID, 'column 1', 'eigenvalue')
        _refused(eng, t, bounds, INVALID, 'column 1', 'eigenvalue', cols=(1, 2))
        # (the plan is refused ahead of the column)
        _refused(eng, t, bounds[::-1], INVALID, 'ascending')
        assert _same(good, eng.history_through_time_eigen(t, bounds, 0, 1))
        assert np.array_equal(eng.expected_counts(0, 1), counts)
    with pytest.raises(hip.HipError, match='sf'):
        with hip.Engine(flat, 1, 4) as eng:
            eng.set_models([(spec, (0.0, rates[1], rates[2]))])
    # one state
    with hip.Engine(flat, 1, 1) as eng:
        one = dict(kind=hip.KIND_EIGEN, pi=np.array([1.0]), d=np.array([0.0]), A=np.array([[1.0]]), Ainv=np.array([[1.0]]))
        eng.set_models([(one, cases.rates(0, 0.0))])
        eng.set_masks(np.ones((1, flat.n_nodes, 1), dtype=np.int8))
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, t, bounds, INVALID, 'k = 1')
        assert np.isfinite(eng.expected_counts()).all()


# ---------------------------------------------------------------------------------------------------------------------
# the front end
# ---------------------------------------------------------------------------------------------------------------------

KEYS = ['bin_length', 'boundaries', 'jumps', 'lineages', 'log_likelihood', 'states', 'times', 'tree_length']


def _annotated_tree():
    tree = read_tree(tcases.NEWICK)
    tips = [tip.name for tip in tree]
    rng = np.random.default_rng(12)
    df = pd.DataFrame({'three': rng.choice(['a', 'b', 'c'], size=len(tips)), 'aa': rng.choice(JTT_STATES[:6], size=len(tips)),
                       'nuc': rng.choice(list('ACGT'), size=len(tips))}, index=tips)
    preannotate_forest([tree], df=df)
    return tree


def _host_view(tree, character, model):
    """(flat, masks the marginal pass runs with: altered where tau == 0)"""
    problem = ml.ForestProblem([tree], character, model.states)
    problem.initialize_allowed_states()
    if 0 == model.tau:
        problem.alter_zero_node_allowed_states()
    return problem.flat, problem.masks.astype(int)


def test_front_end_serves_f81_jtt_and_hky_in_one_call():
    tree = _annotated_tree()
    fs = ForestStats([tree])
    f81 = F81Model(states=np.array(['a', 'b', 'c']), forest_stats=fs, sf=1.2, frequencies=np.array([0.5, 0.3, 0.2]))
    jtt = JTTModel(forest_stats=fs, sf=0.9, tau=0.01)
    hky = _hky(forest_stats=fs, sf=1.3)
    characters, models = ['three', 'aa', 'nuc'], [f81, jtt, hky]
    dates = annotate_dates(ml.get_flat_forest([tree]))
    bounds = np.array([dates.min() - 0.1, 0.2, 0.45, dates.max() + 0.1])
    out = ml.expected_history_through_time_general([tree], characters, models, bounds)
    assert [sorted(x) for x in out] == [KEYS] * 3
    # the F81 family: expected_history_through_time's results bit for bit
    want = ml.expected_history_through_time([tree], 'three', f81, bounds)
    for key in KEYS:
        assert np.array_equal(out[0][key], want[key]), key
    # the eigen models against the restatement
    for i, spec in ((1, jtt.kernel_spec()), (2, hky.eigen_spec())):
        flat, masks = _host_view(tree, characters[i], models[i])
        k = len(models[i].states)
        got = out[i]
        assert list(got['states']) == list(models[i].states) and np.array_equal(got['boundaries'], bounds)
        assert got['times'].shape == (3, k) and got['jumps'].shape == (3, k, k) and got['lineages'].shape == (4, k)
        ref = _check((got['times'], got['jumps'], got['lineages']), flat, masks, (spec, models[i].rate_params()), dates, bounds,
                     'front end ' + characters[i], rows=None)
        assert abs(got['log_likelihood'] - float(ref['loglik'])) < 1e-9 * abs(float(ref['loglik']))
        assert np.abs(got['bin_length'] - np.array([float(x) for x in ref['bin_length']])).max() <= 1e-14 * got['tree_length']
        assert (np.abs(got['times'].sum(axis=1) - got['bin_length']) <= TOLERANCE * got['bin_length']).all()
        assert abs(got['bin_length'].sum() - got['tree_length']) <= 1e-14 * got['tree_length']
    # the masks are restored: the same call gives the same results
    again = ml.expected_history_through_time_general([tree], characters, models, bounds, jumps=False)
    for a, b in zip(again, out):
        assert a['jumps'] is None and a['log_likelihood'] == b['log_likelihood'] and np.array_equal(a['times'], b['times'])
        assert np.array_equal(a['lineages'], b['lineages'])
    # a single character name, an int for equal bins from the earliest root to the latest tip
    single = ml.expected_history_through_time_general([tree], 'aa', jtt, 4)
    assert sorted(single) == KEYS and single['times'].shape == (4, 20)
    assert np.array_equal(single['boundaries'], np.linspace(dates.min(), dates.max(), 5))
    whole = ml.expected_history_general([tree], 'aa', jtt)
    assert single['log_likelihood'] == whole['log_likelihood']
    gross = whole['jumps'].max()
    assert np.abs(single['jumps'].sum(axis=0) - whole['jumps']).max() <= TOLERANCE * 4 * gross
    assert np.abs(single['times'].sum(axis=0) - whole['times']).max() <= TOLERANCE * 4 * whole['times'].max()
