"""
pml_expected_history / Engine.expected_history / ml.expected_history on the device against the decimal restatement of the sums
(tests/expected_history_ref.py), the three identities on the device's own output, bit-reproducibility over schedules,
numberings, columns and calls, and the refusals.

Error measure: every term of every sum is non-negative, so it is the plain relative error |device - exact| / exact per entry;
where the exact value is 0 the device's has to be exactly 0.  TOLERANCE was to be 8 x the worst ratio seen on an MI355X over all
the cases of this file (room for another box's summation order), recorded in profiles/expected_history.txt, and has to stay
below 1e-11, the gradient tests' cap, for their reason: a float64 evaluation of the coefficients stays below 2e-15 on x from
1e-14 to 700, a dropped term or a wrong coefficient is 1e-3 or more.
The worst ratio seen is 7.96e-12 (jumps; times 1.50e-12), in test_branches_of_1e_9_and_1e_12 at k = 65, and 8 x that is
6.4e-11: above the cap.  So TOLERANCE is the cap itself, 1e-11 -- less than the 8 x asked for, 1.26 x the worst case.  That
case's error is not this pass's and not a matter of summation order: it is the rounding of e_n = exp(-mu t'_n) to a double in
the marginal pass, which leaves 1 - e_n of a branch of 1e-12 off by 1e-4 of itself and the small entries of the vectors above
such a branch with it.  The restatement run on the exponentials the device stored (expected_history_ref._vectors_stored)
differs from the exact one by the same 7.96e-12 and 1.50e-12 to three digits, and the device agrees with IT to
STORED_E_TOLERANCE.  Every other case of the file stays below 2.7e-14.
STORED_E_TOLERANCE = 1e-12: each entry is a sum of non-negative terms, a term's factors q_p and v_n carry the rounding of some
twenty levels of k-term sums and products, about a hundred roundings or 1e-14; 1e-12 leaves two digits of room and is five digits
below what a 1 - e_n other than the sweeps' own would show on a branch of 1e-9 (1e-7).

The identities, in float64 on what the device returned, to 1e-12 of the gross of their two sides:
    I1: sum_s times[s] = sum_n L_n;   I2: sum_j jumps[j][i] - sum_j jumps[i][j] = sum_n (q_n[i] - q_p(n)[i]) for every state i;
    I3: sum_n branch_jumps[n] = sum_{i != j} jumps[i][j]
"""
import os

import numpy as np
import pandas as pd
import pytest

import expected_history_ref as href
import loglik_gradient_cases as cases
from conftest import load_golden, GOLDEN
from pastml_amd import hip, ml
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.models.F81Model import F81Model
from pastml_amd.models.HKYModel import HKYModel
from pastml_amd.models.JCModel import JCModel
from pastml_amd.tree import FlatForest, read_tree

pytestmark = pytest.mark.gpu

TOLERANCE = 1e-11
assert TOLERANCE <= 1e-11
STORED_E_TOLERANCE = 1e-12
IDENTITY = 1e-12

DATA = os.path.join(GOLDEN, 'data')
TREE_NWK = os.path.join(DATA, 'Albanian.tree.152tax.tre')
STATES_INPUT = os.path.join(DATA, 'data.txt')


def _model(kind, k, seed, tau):
    return dict(kind=hip.KIND_F81, pi=cases.frequencies(kind, k, seed)), cases.rates(seed, tau)


def _device(flat, masks_cols, models, k, tune=None, cols=None, calls=1, jumps=True, branch_jumps=True, posterior=False):
    """(times, jumps, branch_jumps) of Engine.expected_history, and the posteriors [cols, N, k] behind them if asked for."""
    with hip.Engine(flat, len(models), k, tune=tune) as eng:
        eng.set_models(models)
        eng.set_masks(np.asarray(masks_cols))
        post = eng.marginal_pass(posterior=posterior, lh=False)[1]
        for _ in range(calls):
            out = eng.expected_history(*(cols or ()), jumps=jumps, branch_jumps=branch_jumps)
        return out + (post,) if posterior else out


def _jump_rows(k):
    return None if k <= 65 else [0, 15, 16, 63, 64, k - 17, k - 2, k - 1]


def _check(got, flat, masks, model, label, rows='by k'):
    """One column's (times [k], jumps [k, k], branch_jumps [N]) against the restatement; the ratios are printed, then held."""
    spec, (sf, tau, tf) = model
    times, jumps, branch = got
    k = len(times)
    rows = _jump_rows(k) if rows == 'by k' else rows
    h = href.history(flat, masks, spec['pi'], sf, tau, tf, jump_rows=rows)
    assert np.isfinite(times).all() and np.isfinite(jumps).all() and np.isfinite(branch).all(), label
    assert (np.diag(jumps) == 0).all(), label
    r_times = href.relative_errors(times, h['times']).max()
    r_branch = href.relative_errors(branch, h['branch_jumps']).max()
    r_jumps = max(href.relative_errors(jumps[i], h['jumps'][i]).max() for i in sorted(h['jumps']))
    print('ratio {}: times {:.3g} jumps {:.3g} branch_jumps {:.3g}'.format(label, r_times, r_jumps, r_branch))
    worst = max(r_times, r_jumps, r_branch)
    assert worst <= TOLERANCE, (label, r_times, r_jumps, r_branch)


def _check_identities(got, post, flat, model, label):
    _, (sf, tau, tf) = model
    times, jumps, branch = got
    branches = flat.parent >= 0
    length = ((flat.dist[branches] + tau) * tf).sum()
    assert abs(times.sum() - length) <= IDENTITY * length, (label, 'I1', times.sum(), length)
    inflow, outflow = jumps.sum(axis=0), jumps.sum(axis=1)
    gain, loss = post[branches].sum(axis=0), post[flat.parent[branches]].sum(axis=0)
    gross = inflow + outflow + gain + loss
    assert (np.abs((inflow - outflow) - (gain - loss)) <= IDENTITY * gross).all(), (label, 'I2')
    assert branch[~branches].tolist() == [0.0] * int((~branches).sum()), label
    assert abs(branch.sum() - jumps.sum()) <= IDENTITY * jumps.sum(), (label, 'I3', branch.sum(), jumps.sum())


KS = (2, 3, 4, 5, 16, 17, 63, 64, 65, 130, 256, 257, 512)
CASES = [(kind, k) for kind in ('F81', 'JC') for k in KS]


@pytest.mark.parametrize('shape', cases.SHAPES)
@pytest.mark.parametrize('kind, k', CASES)
def test_device_against_the_reference(kind, k, shape):
    """Every shape at every k, F81 and JC, tau = 0 and tau > 0."""
    i = CASES.index((kind, k))
    flat = cases.forest(shape, seed=i % 3)
    masks = cases.masks(flat, k, i)
    for tau in (0.0, 0.011):
        model = _model(kind, k, i % 4, tau)
        label = '{} k={} {} tau={}'.format(kind, k, shape, tau)
        times, jumps, branch, post = _device(flat, [masks], [model], k, posterior=True)
        _check((times[0], jumps[0], branch[0]), flat, masks, model, label)
        _check_identities((times[0], jumps[0], branch[0]), post[0], flat, model, label)
        if shape == 'zeros' and tau == 0:
            zero = (flat.parent >= 0) & (flat.dist == 0)
            assert zero.any() and (branch[0][zero] == 0).all()


@pytest.mark.parametrize('k', [5, 65])
def test_branches_of_1e_9_and_1e_12(k):
    """(1 - 2 g + e formed directly has no digit left here)"""
    flat = cases.forest('ragged')
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[3::7]] = 1e-9
    flat.dist[branches[5::7]] = 1e-12
    masks = cases.masks(flat, k, 2)
    model = _model('F81', k, 1, 0.0)
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([model])
        eng.set_masks(np.asarray([masks]))
        eng.marginal_pass(posterior=False, lh=False)
        times, jumps, branch = eng.expected_history(branch_jumps=True)
        e = eng.download(hip.BUF_BRANCH_EXP, 0)
    assert (e[flat.parent >= 0] < 1.0).all()
    _check((times[0], jumps[0], branch[0]), flat, masks, model, 'near-zero branches k={}'.format(k))
    # against the marginal pass restated on the exponentials the device stored: what is left is this pass's own arithmetic
    spec, (sf, tau, tf) = model
    h = href.history(flat, masks, spec['pi'], sf, tau, tf, stored_e=e)
    r = max(href.relative_errors(times[0], h['times']).max(), href.relative_errors(branch[0], h['branch_jumps']).max(),
            max(href.relative_errors(jumps[0][i], h['jumps'][i]).max() for i in range(k)))
    print('ratio near-zero branches k={} on the stored exponentials: {:.3g}'.format(k, r))
    assert r <= STORED_E_TOLERANCE, r


@pytest.mark.parametrize('k', [5, 65])
def test_long_branches_whose_exponential_underflows(k):
    flat = cases.forest('ragged')
    masks = cases.masks(flat, k, 4)
    model = _model('F81', k, 2, 0.0)
    spec, (sf, tau, tf) = model
    mu = 1.0 / (1.0 - spec['pi'].dot(spec['pi']))
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[::5]] = 800.0 / (mu * sf * tf)   # (x = mu t' = 800)
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([model])
        eng.set_masks(np.asarray([masks]))
        eng.marginal_pass(posterior=False, lh=False)
        times, jumps, branch = eng.expected_history(branch_jumps=True)
        e = eng.download(hip.BUF_BRANCH_EXP, 0)
    assert (e[branches[::5]] == 0.0).all()
    _check((times[0], jumps[0], branch[0]), flat, masks, model, 'long branches k={}'.format(k))


# (k, ids per piece): the branch pass's 1024, 512 and 256 (history_piece), the jump product's 2048 and 4096 (history_jump_piece;
# pml_launch_history.hip)
PIECES = [(4, 1024), (16, 512), (65, 256), (16, 2048), (65, 4096)]


@pytest.mark.parametrize('k, piece', PIECES)
def test_more_nodes_than_one_piece(k, piece):
    """2 x piece + 37 nodes, once per piece size of the launcher; of the jumps of the largest forests, five rows."""
    flat = FlatForest.random(piece + 19, seed=21, max_arity=2, zero_frac=0.0, n_trees=1)
    assert flat.n_nodes == 2 * piece + 37
    masks = cases.masks(flat, k, 3)
    model = _model('F81', k, 2, 0.0)
    times, jumps, branch = _device(flat, [masks], [model], k)
    rows = None if k * flat.n_nodes <= 70000 else [0, 15, k // 2, k - 2, k - 1]
    _check((times[0], jumps[0], branch[0]), flat, masks, model, 'pieces k={} piece={}'.format(k, piece), rows=rows)


@pytest.mark.parametrize('k', [5, 24, 70])
def test_several_columns_with_their_own_parameters(k):
    flat = cases.forest('forest')
    models = [_model('F81', k, s, 0.01 * (s % 3)) for s in range(5)]
    masks = [cases.masks(flat, k, 10 + s) for s in range(5)]
    times, jumps, branch = _device(flat, masks, models, k)
    for c in range(5):
        _check((times[c], jumps[c], branch[c]), flat, masks[c], models[c], 'k={} column {}'.format(k, c), rows=None)
    # a sub-range of the columns is the same columns
    sub = _device(flat, masks, models, k, cols=(1, 4))
    assert np.array_equal(sub[0], times[1:4]) and np.array_equal(sub[1], jumps[1:4]) and np.array_equal(sub[2], branch[1:4])


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('k, n_tips', [(4, 3000), (24, 1500), (130, 700)])
def test_bits_do_not_depend_on_schedules_numbering_column_or_call(k, n_tips):
    flat = FlatForest.random(n_tips, seed=11, max_arity=3, zero_frac=0.0, n_trees=2)
    masks = cases.masks(flat, k, 1)
    model = _model('F81', k, 1, 0.0)
    base = _device(flat, [masks], [model], k)
    assert all(np.isfinite(x).all() for x in base)
    assert _same(base, _device(flat, [masks], [model], k, calls=2))
    assert _same(base, _device(flat, [masks], [model], k, tune={'NO_SUPER': 1}))
    assert _same(base, _device(flat, [masks], [model], k, tune={'NO_HEIGHT_ORDER': 1}))   # (the caller's numbering kept)
    others = [cases.masks(flat, k, 50 + c) for c in range(6)]
    other_models = [_model('F81', k, c % 4, 0.01 * (c % 2)) for c in range(6)]
    first = _device(flat, [masks] + others, [model] + other_models, k)
    last = _device(flat, others + [masks], other_models + [model], k)
    assert _same([x[0] for x in first], [x[0] for x in base])
    assert _same([x[6] for x in last], [x[0] for x in base])
    assert _same([x[1:] for x in first], [x[:6] for x in last])


@pytest.mark.parametrize('k', [4, 24, 130])
def test_times_have_the_same_bits_whatever_else_is_asked_for(k):
    flat = cases.forest('polytomy')
    masks = cases.masks(flat, k, 5)
    model = _model('F81', k, 3, 0.011)
    full = _device(flat, [masks], [model], k)
    for jumps, branch_jumps in ((False, False), (True, False), (False, True)):
        got = _device(flat, [masks], [model], k, jumps=jumps, branch_jumps=branch_jumps)
        assert np.array_equal(got[0], full[0])
        assert (got[1] is None) == (not jumps) and (got[2] is None) == (not branch_jumps)
        assert got[1] is None or np.array_equal(got[1], full[1])
        assert got[2] is None or np.array_equal(got[2], full[2])


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------

def _refused(eng, status, *words):
    with pytest.raises(hip.HipError) as info:
        eng.expected_history()
    assert info.value.status == status, str(info.value)
    for word in words:
        assert word in str(info.value), str(info.value)


def test_refusals_leave_the_context_answering():
    flat = cases.forest('balanced')
    # no marginal pass
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([_model('F81', 4, 0, 0.0)])
        eng.set_masks(np.asarray([cases.masks(flat, 4, 0)]))
        _refused(eng, hip.PML_ERR_INVALID, 'pml_expected_history', 'marginal')
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts()
        first = eng.expected_history(branch_jumps=True)
        assert all(np.isfinite(x).all() for x in first)
        assert np.array_equal(eng.expected_counts(), counts)   # (the results of the pass stay)
        assert _same(first, eng.expected_history(branch_jumps=True))
    # a model kind other than F81
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([(dict(kind=hip.KIND_HKY, pi=cases.frequencies('F81', 4, 0), kappa=2.0), cases.rates(0, 0.0))])
        eng.set_masks(np.asarray([cases.masks(flat, 4, 0)]))
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, hip.PML_ERR_UNSUPPORTED, 'F81', 'HKY')
        assert np.isfinite(eng.expected_counts()).all()
    # a column whose pi . pi is 1: mu is infinite (every tip in the one state there is, or missing)
    with hip.Engine(flat, 2, 2) as eng:
        eng.set_models([_model('F81', 2, 0, 0.0), (dict(kind=hip.KIND_F81, pi=np.array([1.0, 0.0])), cases.rates(0, 0.0))])
        masks = np.ones((2, flat.n_nodes, 2), dtype=np.int8)
        masks[:, flat.tips[::2], 1] = 0
        eng.set_masks(masks)
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, hip.PML_ERR_INVALID, 'column 1', 'pi . pi')
        assert np.isfinite(eng.expected_history(0, 1)[0]).all()   # (the other column is served)
    # one state
    with hip.Engine(flat, 1, 1) as eng:
        eng.set_models([(dict(kind=hip.KIND_F81, pi=np.array([1.0])), cases.rates(0, 0.0))])
        eng.set_masks(np.ones((1, flat.n_nodes, 1), dtype=np.int8))
        eng.marginal_pass(posterior=False, lh=False)
        _refused(eng, hip.PML_ERR_INVALID, 'k = 1')
        assert np.isfinite(eng.expected_counts()).all()
        _refused(eng, hip.PML_ERR_INVALID, 'k = 1')


def test_front_end_refuses_other_models_by_name():
    flat = cases.forest('balanced')
    roots = flat.to_tree_nodes()
    model = HKYModel(forest_stats=ForestStats(roots), sf=1.0)
    with pytest.raises(NotImplementedError, match='HKY') as info:
        ml.expected_history(roots, 'c', model)
    assert 'PML_ERR_UNSUPPORTED' in str(info.value)


# ---------------------------------------------------------------------------------------------------------------------
# the front end on the Albania tree
# ---------------------------------------------------------------------------------------------------------------------

def _albania():
    zz = load_golden('albania_F81')
    tree = read_tree(TREE_NWK)
    preannotate_forest([tree], df=pd.read_csv(STATES_INPUT, index_col=0, header=0)[['Country']])
    return tree, zz


def _host_view(tree, model):
    """(flat, masks the marginal pass runs with: altered where tau == 0)"""
    problem = ml.ForestProblem([tree], 'Country', model.states)
    problem.initialize_allowed_states()
    if 0 == model.tau:
        problem.alter_zero_node_allowed_states()
    return problem.flat, problem.masks.astype(int)


def test_front_end_on_the_albania_tree():
    tree, zz = _albania()
    stats = ForestStats([tree])
    f81 = F81Model(states=zz['opt_states'], forest_stats=stats, sf=float(zz['opt_sf']), frequencies=zz['opt_frequencies'])
    jc = JCModel(states=zz['opt_states'], forest_stats=stats, sf=float(zz['opt_sf']))
    k = len(f81.states)
    before = ml.loglikelihood_gradient([tree], 'Country', f81)['log_likelihood']
    out = ml.expected_history([tree], 'Country', f81)
    assert sorted(out) == ['jumps', 'log_likelihood', 'states', 'times', 'tree_length']
    both = ml.expected_history([tree], ['Country', 'Country'], [f81, jc], branch_jumps=True)
    assert sorted(both[0]) == sorted(both[1]) == ['branch_jumps', 'jumps', 'log_likelihood', 'states', 'times', 'tree_length']
    assert np.array_equal(both[0]['times'], out['times']) and np.array_equal(both[0]['jumps'], out['jumps'])
    assert both[0]['log_likelihood'] == out['log_likelihood'] == before
    # the masks are restored: the same forest gives the ln L it gave before
    assert ml.loglikelihood_gradient([tree], 'Country', f81)['log_likelihood'] == before
    for model, result, label in ((f81, both[0], 'Albania F81'), (jc, both[1], 'Albania JC')):
        flat, masks = _host_view(tree, model)
        assert list(result['states']) == list(model.states)
        assert result['times'].shape == (k,) and result['jumps'].shape == (k, k) and result['branch_jumps'].shape == (flat.n_nodes,)
        assert abs(result['times'].sum() - result['tree_length']) <= 1e-12 * result['tree_length']
        assert (np.diag(result['jumps']) == 0).all()
        sf, tau, tf = model.rate_params()
        h = href.history(flat, masks, model.frequencies, sf, tau, tf)
        assert abs(result['tree_length'] - float(h['tree_length'])) <= 1e-14 * result['tree_length']
        assert abs(result['log_likelihood'] - float(h['loglik'])) < 1e-9 * abs(float(h['loglik']))
        _check((result['times'], result['jumps'], result['branch_jumps']), flat, masks,
               (dict(pi=np.asarray(model.frequencies, dtype=np.float64)), (sf, tau, tf)), label, rows=None)
