"""
pml_expected_history_eigen / Engine.expected_history_eigen / ml.expected_history_general on the device against the decimal
restatement of the sums (tests/expected_history_eigen_ref.py), the three identities on the device's own output,
bit-reproducibility over columns, calls and what is asked for, the P(t) window, and the refusals.

Error measure: |device - exact| / (the largest |entry| of the exact array), per output (times, the jump rows held, branch_jumps):
the sums have mixed signs, so the plain per-entry relative error of the F81 tests does not apply.  TOLERANCE is 8 x the worst
ratio seen on an MI355X over all the cases of this file (room for another box's summation order), recorded in
profiles/expected_history_eigen.txt, and must not exceed 1e-9: a dropped term or a wrong coefficient shows at 1e-3 or more.
The worst ratio seen is 2.21e-12 (jumps; branch_jumps 1.48e-12, times 2.93e-13), in test_branches_of_1e_9_and_1e_12 at k = 61;
next come the F81 model as an eigen model at k = 65 on the polytomy forest (1.55e-12 against the restatement, 1.77e-12 against the
F81 entry) and forest S at k = 128 (5.92e-13).  Every case below 33 states stays under 2e-13.  8 x 2.21e-12 = 1.77e-11 is under the
1e-9 cap.

The identities, in float64 on what the device returned, to TOLERANCE of the gross of their two sides:
    I1: sum_s times[s] = sum_n L_n;   I2: sum_j jumps[j][i] - sum_j jumps[i][j] = sum_n (q_n[i] - q_p(n)[i]) for every state i;
    I3: sum_n branch_jumps[n] = sum_{i != j} jumps[i][j]
"""
import os

import numpy as np
import pandas as pd
import pytest

import eigen_shape_cases as shapes
import expected_history_eigen_ref as eref
import loglik_gradient_cases as cases
from conftest import load_golden, GOLDEN
from pastml_amd import hip, ml
from pastml_amd.annotation import ForestStats, preannotate_forest
from pastml_amd.models.CustomRatesModel import CustomRatesModel
from pastml_amd.models.F81Model import F81Model
from pastml_amd.models.HKYModel import HKYModel
from pastml_amd.tree import FlatForest, read_tree
from test_gpu_parity import random_spec

pytestmark = pytest.mark.gpu

WORST_SEEN = 2.21e-12   # near-zero branches k=61, jumps (profiles/expected_history_eigen.txt)
TOLERANCE = 8 * WORST_SEEN
assert TOLERANCE <= 1e-9

DATA = os.path.join(GOLDEN, 'data')
TREE_NWK = os.path.join(DATA, 'Albanian.tree.152tax.tre')
STATES_INPUT = os.path.join(DATA, 'data.txt')
NUCLEOTIDES = 'tree.152taxa.sf_0.5.A_0.6.C_0.15.G_0.2.T_0.05'
PIECE = 512   # PML_HEIG_PIECE


def _device(flat, masks_cols, models, k, cols=None, calls=1, jumps=True, branch_jumps=True, posterior=False, window=0, tune=None):
    """(times, jumps, branch_jumps) of Engine.expected_history_eigen, and the posteriors [cols, N, k] behind them if asked for."""
    with hip.Engine(flat, len(models), k, tune=tune) as eng:
        eng.set_models(models)
        if window:
            eng.pij_window_set(window)
        eng.set_masks(np.asarray(masks_cols))
        post = eng.marginal_pass(posterior=posterior, lh=False)[1]
        for _ in range(calls):
            out = eng.expected_history_eigen(*(cols or ()), jumps=jumps, branch_jumps=branch_jumps)
        if window:
            assert eng.pij_window_info()[0] == window and eng.pij_window_info()[2] == 0
        return out + (post,) if posterior else out


def _jump_rows(k):
    return None if k <= 65 else [0, 15, 16, 63, 64, k - 17, k - 2, k - 1]


def _ratios(got, h):
    times, jumps, branch = got
    rows = sorted(h['jumps'])
    r_jumps = eref.scaled_errors(np.concatenate([jumps[i] for i in rows]), [x for i in rows for x in h['jumps'][i]]).max()
    return eref.scaled_errors(times, h['times']).max(), r_jumps, eref.scaled_errors(branch, h['branch_jumps']).max()


def _check(got, flat, masks, model, label, rows='by k', h=None):
    """One column's (times [k], jumps [k, k], branch_jumps [N]) against the restatement; the ratios are printed, then held."""
    spec, (sf, tau, tf) = model
    times, jumps, branch = got
    rows = _jump_rows(len(times)) if rows == 'by k' else rows
    if h is None:
        h = eref.history(flat, masks, spec, sf, tau, tf, jump_rows=rows)
    for x in got:
        assert np.isfinite(x).all() and (x >= 0).all(), label
    assert (np.diag(jumps) == 0).all(), label
    assert (branch[flat.parent < 0] == 0).all(), label
    r_times, r_jumps, r_branch = _ratios(got, h)
    print('ratio {}: times {:.3g} jumps {:.3g} branch_jumps {:.3g}'.format(label, r_times, r_jumps, r_branch))
    assert max(r_times, r_jumps, r_branch) <= TOLERANCE, (label, r_times, r_jumps, r_branch)
    return h


def _check_identities(got, post, flat, model, label):
    _, (sf, tau, tf) = model
    times, jumps, branch = got
    branches = flat.parent >= 0
    length = ((flat.dist[branches] + tau) * tf).sum()
    assert abs(times.sum() - length) <= TOLERANCE * length, (label, 'I1', times.sum(), length)
    inflow, outflow = jumps.sum(axis=0), jumps.sum(axis=1)
    gain, loss = post[branches].sum(axis=0), post[flat.parent[branches]].sum(axis=0)
    gross = inflow + outflow + gain + loss
    assert (np.abs((inflow - outflow) - (gain - loss)) <= TOLERANCE * gross).all(), (label, 'I2')
    assert abs(branch.sum() - jumps.sum()) <= TOLERANCE * jumps.sum(), (label, 'I3', branch.sum(), jumps.sum())


KS = (2, 4, 5, 15, 16, 17, 20, 32, 33, 61, 64, 65, 128, 129, 256)


@pytest.mark.parametrize('k', KS)
def test_device_against_the_reference(k):
    """Forest S at every k of the MFMA tile and LDS boundaries: both columns with their own models, rates and masks; up to 20
    states also with tau = 0 and tau = 0.011 in both."""
    b = shapes.build(k, 'S')
    flat = b['flat']
    variants = [('own', b['rates'])]
    if k <= 20:
        variants += [('tau={}'.format(tau), [(sf, tau, tf) for sf, _, tf in b['rates']]) for tau in (0.0, 0.011)]
    for name, rates in variants:
        models = list(zip(b['specs'], rates))
        times, jumps, branch, post = _device(flat, b['masks'], models, k, posterior=True)
        for c in range(2):
            label = 'S k={} column {} {}'.format(k, c, name)
            got = (times[c], jumps[c], branch[c])
            _check(got, flat, b['masks'][c], models[c], label)
            _check_identities(got, post[c], flat, models[c], label)


# ---------------------------------------------------------------------------------------------------------------------
# degenerate and near-degenerate eigenvalues
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', cases.SHAPES)
@pytest.mark.parametrize('k', [4, 5, 65])
def test_f81_model_as_eigen_model(k, shape):
    """Every non-zero eigenvalue equal: against the restatement, and against the F81 family's own entry on an F81 context (the two
    paths share no code)."""
    i = [4, 5, 65].index(k)
    flat = cases.forest(shape, seed=i)
    masks = cases.masks(flat, k, i)
    pi = cases.frequencies('F81', k, i)
    rates = cases.rates(i, 0.0)
    model = (eref.f81_as_eigen(pi), rates)
    label = 'F81 as eigen k={} {}'.format(k, shape)
    times, jumps, branch, post = _device(flat, [masks], [model], k, posterior=True)
    got = (times[0], jumps[0], branch[0])
    _check(got, flat, masks, model, label, rows=None)
    _check_identities(got, post[0], flat, model, label)
    if shape == 'zeros':
        zero = (flat.parent >= 0) & (flat.dist == 0)
        assert zero.any() and (branch[0][zero] == 0).all()
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([(dict(kind=hip.KIND_F81, pi=pi), rates)])
        eng.set_masks(np.asarray([masks]))
        eng.marginal_pass(posterior=False, lh=False)
        f81 = eng.expected_history(branch_jumps=True)
    r = [np.abs(x[0] - y).max() / np.abs(x[0]).max() for x, y in zip(f81, got)]
    print('ratio {} against the F81 entry: times {:.3g} jumps {:.3g} branch_jumps {:.3g}'.format(label, *r))
    assert max(r) <= TOLERANCE, (label, r)


def _hky(kappa, forest_stats=None, sf=1.3):
    return HKYModel(forest_stats=forest_stats, sf=sf, frequencies=np.array([0.1, 0.35, 0.05, 0.5]), kappa=kappa)


@pytest.mark.parametrize('kappa', [1.0, 1.0 + 1e-9])
def test_hky_as_eigen_model_at_and_next_to_a_repeated_eigenvalue(kappa):
    flat = cases.forest('polytomy')
    masks = cases.masks(flat, 4, 6)
    model = (_hky(kappa).eigen_spec(), cases.rates(1, 0.011))
    times, jumps, branch, post = _device(flat, [masks], [model], 4, posterior=True)
    got = (times[0], jumps[0], branch[0])
    _check(got, flat, masks, model, 'HKY kappa={!r}'.format(kappa))
    _check_identities(got, post[0], flat, model, 'HKY kappa={!r}'.format(kappa))


# ---------------------------------------------------------------------------------------------------------------------
# branch lengths
# ---------------------------------------------------------------------------------------------------------------------

def _eigen_model(k, tau=0.0):
    b = shapes.build(k, 'S')
    return b['specs'][0], (b['rates'][0][0], tau, 1.0)


def _one_column(flat, masks, model, k, label):
    times, jumps, branch, post = _device(flat, [masks], [model], k, posterior=True)
    got = (times[0], jumps[0], branch[0])
    _check(got, flat, masks, model, label)
    _check_identities(got, post[0], flat, model, label)
    return got


@pytest.mark.parametrize('k', [5, 61])
def test_branches_of_1e_9_and_1e_12(k):
    """(every pair takes the series of phi there)"""
    flat = cases.forest('ragged')
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[3::7]] = 1e-9
    flat.dist[branches[5::7]] = 1e-12
    _one_column(flat, cases.masks(flat, k, 2), _eigen_model(k), k, 'near-zero branches k={}'.format(k))


@pytest.mark.parametrize('k', [5, 61])
def test_long_branches_whose_exponentials_underflow(k):
    """max |d| t' = 800: every E but the stationary one is 0"""
    flat = cases.forest('ragged')
    model = _eigen_model(k)
    spec, (sf, tau, tf) = model
    d = np.sort(np.abs(spec['d']))
    branches = np.flatnonzero(flat.parent >= 0)
    flat.dist[branches[::5]] = 800.0 / (d[-1] * sf * tf)
    assert np.exp(-d[1] * 800.0 / d[-1]) < 1e-3 or k == 5
    _one_column(flat, cases.masks(flat, k, 4), model, k, 'long branches k={}'.format(k))


@pytest.mark.parametrize('k', [5, 61])
def test_zero_branches_add_nothing(k):
    flat = cases.forest('zeros')
    got = _one_column(flat, cases.masks(flat, k, 3), _eigen_model(k), k, 'zero branches k={}'.format(k))
    zero = (flat.parent >= 0) & (flat.dist == 0)
    assert zero.any() and (got[2][zero] == 0).all()


def test_more_nodes_than_one_piece():
    """2 x piece + 37 nodes; the launcher has one piece size (PML_HEIG_PIECE), used from two states on."""
    flat = FlatForest.random(PIECE + 19, seed=21, max_arity=2, zero_frac=0.0, n_trees=1)
    assert flat.n_nodes == 2 * PIECE + 37
    _one_column(flat, cases.masks(flat, 2, 3), _eigen_model(2), 2, 'pieces k=2 piece={}'.format(PIECE))


# ---------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _random_models(k, n, seed):
    rng = np.random.default_rng(seed)
    return [(random_spec('EIGEN', k, rng), (float(rng.uniform(0.5, 3)), 0.01 * (c % 2), 1.0 - 0.05 * (c % 2))) for c in range(n)]


@pytest.mark.parametrize('k, n_tips', [(4, 1500), (20, 1500), (130, 700)])
def test_bits_do_not_depend_on_column_or_call(k, n_tips):
    flat = FlatForest.random(n_tips, seed=11, max_arity=3, zero_frac=0.0, n_trees=2)
    masks = cases.masks(flat, k, 1)
    (model,) = _random_models(k, 1, 70 + k)
    base = _device(flat, [masks], [model], k)
    assert all(np.isfinite(x).all() for x in base)
    assert _same(base, _device(flat, [masks], [model], k, calls=2))
    others = [cases.masks(flat, k, 50 + c) for c in range(6)]
    other_models = _random_models(k, 6, 170 + k)
    first = _device(flat, [masks] + others, [model] + other_models, k)
    last = _device(flat, others + [masks], other_models + [model], k)
    assert _same([x[0] for x in first], [x[0] for x in base])
    assert _same([x[6] for x in last], [x[0] for x in base])
    assert _same([x[1:] for x in first], [x[:6] for x in last])
    # a sub-range of the columns is the same columns
    five = first
    sub = _device(flat, [masks] + others, [model] + other_models, k, cols=(1, 4))
    assert _same(sub, [x[1:4] for x in five])


@pytest.mark.parametrize('k', [4, 20, 130])
def test_times_have_the_same_bits_whatever_else_is_asked_for(k):
    flat = cases.forest('polytomy')
    masks = cases.masks(flat, k, 5)
    (model,) = _random_models(k, 1, 270 + k)
    full = _device(flat, [masks], [model], k)
    for jumps, branch_jumps in ((False, False), (True, False), (False, True)):
        got = _device(flat, [masks], [model], k, jumps=jumps, branch_jumps=branch_jumps)
        assert np.array_equal(got[0], full[0])
        assert (got[1] is None) == (not jumps) and (got[2] is None) == (not branch_jumps)
        assert got[1] is None or np.array_equal(got[1], full[1])
        assert got[2] is None or np.array_equal(got[2], full[2])


def test_window_leaves_no_batch_and_the_same_bits():
    k = 40
    flat = cases.forest('polytomy')
    masks = [cases.masks(flat, k, 7), cases.masks(flat, k, 8)]
    models = _random_models(k, 2, 340)
    plain = _device(flat, masks, models, k)
    windowed = _device(flat, masks, models, k, window=int(flat.n_children.max()))
    assert _same(plain, windowed)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------

def _refused(eng, status, *words, **kwargs):
    with pytest.raises(hip.HipError) as info:
        eng.expected_history_eigen(*kwargs.get('cols', ()))
    assert info.value.status == status, str(info.value)
    for word in words:
        assert word in str(info.value), str(info.value)


def test_refusals_leave_the_context_answering():
    flat = cases.forest('balanced')
    masks = np.asarray([cases.masks(flat, 4, 0)])
    eigen = _random_models(4, 2, 5)
    # no marginal pass
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models(eigen[:1])
        eng.set_masks(masks)
        _refused(eng, hip.PML_ERR_INVALID, 'pml_expected_history_eigen', 'marginal')
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts()
        first = eng.expected_history_eigen(branch_jumps=True)
        assert all(np.isfinite(x).all() for x in first)
        assert np.array_equal(eng.expected_counts(), counts)   # (the results of the pass stay)
        assert _same(first, eng.expected_history_eigen(branch_jumps=True))
    # an F81 context: pointed to pml_expected_history
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([(dict(kind=hip.KIND_F81, pi=cases.frequencies('F81', 4, 0)), cases.rates(0, 0.0))])
        eng.set_masks(masks)
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts()
        _refused(eng, hip.PML_ERR_UNSUPPORTED, 'F81', 'pml_expected_history ')
        assert np.array_equal(eng.expected_counts(), counts)
    # an HKY context: pointed to the eigen form of the model
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([(dict(kind=hip.KIND_HKY, pi=cases.frequencies('F81', 4, 0), kappa=2.0), cases.rates(0, 0.0))])
        eng.set_masks(masks)
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts()
        _refused(eng, hip.PML_ERR_UNSUPPORTED, 'HKY', 'as an eigen model')
        assert np.array_equal(eng.expected_counts(), counts)
    # a column whose eigenvalues are not finite (-inf: its exponentials are 0, the sweeps still run): the message names the column,
    # and a sub-range call serves the other one.  (A scaling factor that is not finite and positive never gets as far as this
    # entry: pml_model_set_eigen refuses it.)
    spec, rates = eigen[1]
    bad = (dict(spec, d=np.where(np.arange(4) == 2, -np.inf, spec['d'])), rates)
    with hip.Engine(flat, 2, 4) as eng:
        eng.set_models([eigen[0], eigen[0]])
        eng.set_masks(np.concatenate([masks, masks]))
        eng.marginal_pass(posterior=False, lh=False)
        good = eng.expected_history_eigen(0, 1)
        eng.set_models([bad], col_begin=1)
        eng.marginal_pass(posterior=False, lh=False)
        counts = eng.expected_counts(0, 1)
        _refused(eng, hip.PML_ERR_INVALID, 'column 1', 'eigenvalue')
        _refused(eng, hip.PML_ERR_INVALID, 'column 1', 'eigenvalue', cols=(1, 2))
        assert _same(good, eng.expected_history_eigen(0, 1))
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
        _refused(eng, hip.PML_ERR_INVALID, 'k = 1')
        assert np.isfinite(eng.expected_counts()).all()
        _refused(eng, hip.PML_ERR_INVALID, 'k = 1')


# ---------------------------------------------------------------------------------------------------------------------
# the front end
# ---------------------------------------------------------------------------------------------------------------------

def _albania():
    zz = load_golden('albania_F81')
    tree = read_tree(TREE_NWK)
    preannotate_forest([tree], df=pd.read_csv(STATES_INPUT, index_col=0, header=0)[['Country']])
    return tree, zz


def _host_view(tree, character, model):
    """(flat, masks the marginal pass runs with: altered where tau == 0)"""
    problem = ml.ForestProblem([tree], character, model.states)
    problem.initialize_allowed_states()
    if 0 == model.tau:
        problem.alter_zero_node_allowed_states()
    return problem.flat, problem.masks.astype(int)


KEYS = ['branch_jumps', 'jumps', 'log_likelihood', 'states', 'times', 'tree_length']


def test_front_end_f81_family_is_expected_history_bit_for_bit():
    tree, zz = _albania()
    f81 = F81Model(states=zz['opt_states'], forest_stats=ForestStats([tree]), sf=float(zz['opt_sf']),
                   frequencies=zz['opt_frequencies'])
    want = ml.expected_history([tree], 'Country', f81, branch_jumps=True)
    got = ml.expected_history_general([tree], 'Country', f81, branch_jumps=True)
    assert sorted(got) == sorted(want) == KEYS
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    assert 'branch_jumps' not in ml.expected_history_general([tree], ['Country'], [f81])[0]


def _front_end(tree, character, model, spec, label):
    out = ml.expected_history_general([tree], character, model, branch_jumps=True)
    assert sorted(out) == KEYS
    assert out['log_likelihood'] < -1.0   # (the annotation is there)
    # the masks are restored: the same forest gives the ln L it gave before
    assert ml.expected_history_general([tree], character, model)['log_likelihood'] == out['log_likelihood']
    flat, masks = _host_view(tree, character, model)
    k = len(model.states)
    assert list(out['states']) == list(model.states)
    assert out['times'].shape == (k,) and out['jumps'].shape == (k, k) and out['branch_jumps'].shape == (flat.n_nodes,)
    assert abs(out['times'].sum() - out['tree_length']) <= TOLERANCE * out['tree_length']
    sf, tau, tf = model.rate_params()
    h = _check((out['times'], out['jumps'], out['branch_jumps']), flat, masks, (spec, (sf, tau, tf)), label, rows=None)
    assert abs(out['tree_length'] - float(h['tree_length'])) <= 1e-14 * out['tree_length']
    assert abs(out['log_likelihood'] - float(h['loglik'])) < 1e-9 * abs(float(h['loglik']))
    return out


def test_front_end_custom_rates_on_the_albania_tree():
    tree, zz = _albania()
    states = np.array(zz['opt_states'])
    assert len(states) == 5
    fs = ForestStats([tree])
    # (the file's matrix under the character's own state names and the stored frequencies)
    model = CustomRatesModel(forest_stats=fs, sf=1.0 / fs.avg_nonzero_brlen, states=states,
                             rate_matrix=np.loadtxt(os.path.join(DATA, 'custom_rates_k5.txt')), frequencies=zz['opt_frequencies'])
    _front_end(tree, 'Country', model, model.kernel_spec(), 'Albania CUSTOM_RATES')


def test_front_end_hky_on_the_nucleotide_tree():
    tree = read_tree(os.path.join(DATA, NUCLEOTIDES + '.nwk'))
    df = pd.read_csv(os.path.join(DATA, NUCLEOTIDES + '.pastml.tab'), index_col=0, header=0, sep='\t')[['ACR']]
    preannotate_forest([tree], df=df.loc[[tip.name for tip in tree]])
    fs = ForestStats([tree])
    model = HKYModel(forest_stats=fs, sf=0.5, frequencies=np.array([0.6, 0.15, 0.2, 0.05]), kappa=4.0)
    out = _front_end(tree, 'ACR', model, model.eigen_spec(), 'nucleotides HKY')
    with pytest.raises(NotImplementedError, match='HKY'):
        ml.expected_history([tree], 'ACR', model)
    assert out['log_likelihood'] < -1.0
