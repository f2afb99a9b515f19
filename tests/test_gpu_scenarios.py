"""
Scenarios from the joint posterior on the device (pml_sample_scenarios, pastml_amd.utilities.scenario_sampler) draw for draw
against their restatement (tests/scenario_ref.py), which reads the device's own inputs: the bottom-up vectors and posteriors
(BUF_BU / BUF_POSTERIOR), E (BUF_BRANCH_EXP) or the P(t) batch, the masks the pass ran with, pi as handed to set_models.

Every state is compared with the restatement conditioned on the device's parent states (a failure names one node).  The
policy is that of test_gpu_sampler_exact.py: a device draw may differ from the restated one only if the restatement lists it as
near (its scaled uniform within 1e-12 W of a boundary of its table), then only to the adjacent state, at most 2 per case; the
restatement's own near list must have at most 2 entries for the fixed seeds.

The exact cases: every model on every tree at 250 repetitions (a ragged last tuple), and every model on the forest at 1 and
1024 repetitions.
"""
import numpy as np
import pytest
from scipy import stats

import scenario_ref as ref
from oracle import pastml_oracle as orc
from pastml_amd import hip, ml
from pastml_amd.annotation import ForestStats
from pastml_amd.batch import CharacterBatch, words_from_masks, masks_from_words
from pastml_amd.models._closed_form import F81Model
from pastml_amd.models._eigen import CustomRatesModel, JTTModel
from pastml_amd.models.JTTModel import JTT_STATES
from pastml_amd.tree import FlatForest
from pastml_amd.utilities.scenario_sampler import sample_scenarios, scenario_transition_counts

pytestmark = pytest.mark.gpu

MAX_FLIPS = 2


# ---------------------------------------------------------------------------------------------------------------------
# forests, models, masks
# ---------------------------------------------------------------------------------------------------------------------

def _caterpillar(depth, seed=5):
    n = 2 * depth + 1
    parent = np.full(n, -1, dtype=np.int32)
    n_children = np.zeros(n, dtype=np.int32)
    first_child = np.zeros(n, dtype=np.int32)
    spine = [0] + [2 * d - 1 for d in range(1, depth + 1)]
    for d in range(depth):
        p = spine[d]
        n_children[p] = 2
        first_child[p] = 2 * d + 1
        parent[2 * d + 1] = p
        parent[2 * d + 2] = p
    dist = np.random.default_rng(seed).uniform(0.001, 0.2, size=n)
    return FlatForest(parent, n_children, first_child, dist, np.array([0]))


TREES = ['forest300', 'caterpillar200', 'zero64', 'single']


def _forest(name):
    if name == 'forest300':
        return FlatForest.random(300, seed=3, max_arity=4, n_trees=3)        # polytomies, 3 roots; renumbered by the library
    if name == 'caterpillar200':
        return _caterpillar(199)                                             # 200 tips, deep: rescaled bottom-up rows
    if name == 'zero64':
        return FlatForest.random(64, seed=8, max_arity=3, zero_frac=0.3)     # zero-length internal and tip branches
    return FlatForest([-1], [0], [1], [0.0], [0])                            # a single tip


def _spec(kind, k, flat, seed=0, sf=1.3, tau=0.1):
    """(spec, (sf, tau, tau_factor)) as set_models takes it."""
    rng = np.random.default_rng(1000 + 17 * k + seed)
    rates = (sf, tau, 1.0)
    if kind == 'F81':
        return dict(kind=hip.KIND_F81, pi=rng.dirichlet(np.ones(k) * 2)), rates
    if kind == 'HKY':
        return dict(kind=hip.KIND_HKY, pi=rng.dirichlet(np.ones(4) * 3), kappa=2.0 + seed), rates
    if kind == 'CR':
        pi = rng.dirichlet(np.ones(k) * 3)
        r = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
        d, a, ainv = orc.diagonalise(pi, r + r.T)
        return dict(kind=hip.KIND_EIGEN, pi=pi, d=d, A=a, Ainv=ainv), rates
    if kind == 'JC':
        return dict(kind=hip.KIND_F81, pi=np.full(k, 1.0 / k)), rates
    if kind == 'JTT':   # (the fixed rates and frequencies of the model; its forest statistics play no part in the spec)
        return JTTModel(forest_stats=ForestStats(FlatForest.balanced(3).to_tree_nodes()), sf=sf).kernel_spec(), rates
    raise ValueError(kind)


def _tip_masks(flat, k, seed):
    """Tips observed, missing (all states) or ambiguous (2-3 states)."""
    rng = np.random.default_rng(seed)
    m = np.ones((flat.n_nodes, k), dtype=np.int8)
    for t in flat.tips:
        r = rng.random()
        if r < 0.15 or k == 1:
            continue
        m[t] = 0
        if r < 0.3:
            m[t, rng.choice(k, size=min(k, int(rng.integers(2, 4))), replace=False)] = 1
        else:
            m[t, rng.integers(k)] = 1
    return m


def _masks(flat, k, seed, tree='forest300'):
    """The masks a pass runs with.  zero64 (tau = 0): observed tips, then the zero-branch alteration of the library's own host
    code -- the clashing members of a zero-length cluster get the union of their states.  Elsewhere some internal nodes
    are restricted to half the states as well."""
    if tree == 'zero64':
        rng = np.random.default_rng(seed)
        m = np.ones((flat.n_nodes, k), dtype=np.int8)
        m[flat.tips] = 0
        m[flat.tips, rng.integers(0, min(k, 3), size=len(flat.tips))] = 1
        batch = CharacterBatch(flat, k, 1)
        annotated = np.zeros(flat.n_nodes, dtype=bool)
        annotated[flat.tips] = True
        batch.set_annotation(0, np.where(annotated[:, None], words_from_masks(m, k), np.uint64(0)), annotated)
        batch.initialize_allowed_states()
        altered = batch.alter(np.ones(1, dtype=bool))[0]
        assert altered.any(), 'no node was altered: the case does not test what it says'
        return masks_from_words(batch.masks[0], k).astype(np.int8)
    m = _tip_masks(flat, k, seed)
    if k > 2 and tree == 'forest300':
        rng = np.random.default_rng(seed + 1)
        internal = np.flatnonzero(flat.n_children > 0)
        for n in internal[rng.random(len(internal)) < 0.2]:
            m[n] = 0
            m[n, rng.choice(k, size=k // 2, replace=False)] = 1
    return m


# ---------------------------------------------------------------------------------------------------------------------
# device run and comparison
# ---------------------------------------------------------------------------------------------------------------------

def _marginal_pass(eng, models, masks):
    eng.set_models(models)
    eng.set_masks(masks)
    eng.bottom_up(True)
    eng.top_down_marginals()


def _vectors(eng, spec, col):
    v = dict(bu=eng.download(hip.BUF_BU, col), post=eng.download(hip.BUF_POSTERIOR, col))
    if spec['kind'] == hip.KIND_F81:
        v['inputs'] = dict(E=eng.download(hip.BUF_BRANCH_EXP, col))
    else:
        v['inputs'] = dict(P=eng.pij_batch(copy_out=True)[col])
    return v


def _sample(flat, models, k, masks, n_rep, seed, col=0, rep_offset=0, tune=None):
    with hip.Engine(flat, len(models), k, tune=tune) as eng:
        _marginal_pass(eng, models, masks)
        dev, fallen = eng.sample_scenarios(n_rep, seed, rep_offset=rep_offset, col=col)
        v = _vectors(eng, models[col][0], col)
    assert dev.dtype == (np.uint8 if k <= 256 else np.uint16) and dev.shape == (flat.n_nodes, n_rep)
    return dev, fallen, v


def _check(flat, dev, fallen, v, mask, pi, seed, rep_offset, label):
    n_rep = dev.shape[1]
    r = ref.scenarios(flat, mask, v['bu'], v['post'], pi, seed, n_rep, rep_offset, parent_states=dev, **v['inputs'])
    assert len(r['near']) <= MAX_FLIPS, '{}: the restatement lists {} near draws: pick another seed'.format(label, len(r['near']))
    near = {(n, rep) for n, rep, _ in r['near']}
    bad = np.argwhere(r['states'] != dev)
    flips = [(int(n), int(rep)) for n, rep in bad
             if (int(n), int(rep)) in near and abs(int(dev[n, rep]) - int(r['states'][n, rep])) == 1]
    print('{}: {} near draws, {} flips, {} other differences, n_fallback {}'.format(label, len(near), len(flips),
                                                                                  len(bad) - len(flips), fallen))
    assert len(bad) == len(flips), '{}: {} states differ from the restatement given the device parents; first (node, rep, ' \
        'device, restated): {}'.format(label, len(bad), [(int(n), int(q), int(dev[n, q]), int(r['states'][n, q])) for n, q in bad[:8]])
    assert len(flips) <= MAX_FLIPS, '{}: {} near-boundary flips'.format(label, len(flips))
    # invariants: no fallback, every state inside the node's mask, single-state nodes constant
    assert fallen == 0 and r['n_fallback'] == 0, label
    assert np.all(np.asarray(mask)[np.arange(flat.n_nodes)[:, None], dev.astype(np.int64)] == 1), label
    single = np.flatnonzero(np.asarray(mask).sum(axis=1) == 1)
    assert np.all(dev[single] == np.argmax(np.asarray(mask)[single], axis=1)[:, None]), label


def _case(tree, kind, k, n_rep, seed, rep_offset=0):
    flat = _forest(tree)
    models = [_spec(kind, k, flat, tau=0.0 if tree == 'zero64' else 0.1)]
    k = len(models[0][0]['pi'])
    masks = _masks(flat, k, 7 * k + 1, tree)[None]
    dev, fallen, v = _sample(flat, models, k, masks, n_rep, seed, rep_offset=rep_offset)
    _check(flat, dev, fallen, v, masks[0], models[0][0]['pi'], seed, rep_offset, '{} {} k={} n_rep={}'.format(tree, kind, k, n_rep))


# F81: 67 states = two mask words and a second scan chunk, 300 = uint16; CR 130: the cumulative rows in the scratch buffer
MODELS = [('F81', 4), ('F81', 67), ('F81', 300), ('JC', 5), ('HKY', 4), ('JTT', 20), ('CR', 7), ('CR', 130)]
MODEL_IDS = ['{}-k{}'.format(*c) for c in MODELS]


@pytest.mark.parametrize('tree', TREES)
@pytest.mark.parametrize('kind,k', MODELS, ids=MODEL_IDS)
def test_scenarios_exact(kind, k, tree):
    _case(tree, kind, k, 250, (5 << 32) + 1000 * k + len(tree), rep_offset=3)


@pytest.mark.parametrize('n_rep', [1, 1024])
@pytest.mark.parametrize('kind,k', MODELS, ids=MODEL_IDS)
def test_scenarios_exact_repetitions(kind, k, n_rep):
    _case('forest300', kind, k, n_rep, 4242 + k + n_rep)


# ---------------------------------------------------------------------------------------------------------------------
# chunking and numbering
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind,k', [('F81', 6), ('CR', 7)])
def test_scenarios_chunks_seeds_columns_and_numbering(kind, k):
    flat = _forest('forest300')
    models = [_spec(kind, k, flat, seed=c, sf=0.8 + 0.5 * c, tau=0.02 * (c + 1)) for c in range(2)]
    masks = np.stack([_masks(flat, k, 40 + c) for c in range(2)])
    seed, n_rep = 31337, 300
    with hip.Engine(flat, 2, k) as eng:
        _marginal_pass(eng, models, masks)
        assert not np.array_equal(eng.node_order(), np.arange(flat.n_nodes)), 'the library does not renumber this forest'
        whole, _ = eng.sample_scenarios(n_rep, seed, col=1)
        # calls with rep_offset 0 / 6 / 130 make up one call, bit for bit
        parts = [eng.sample_scenarios(c, seed, rep_offset=o, col=1)[0] for o, c in ((0, 6), (6, 124), (130, n_rep - 130))]
        assert np.array_equal(np.concatenate(parts, axis=1), whole)
        other, _ = eng.sample_scenarios(n_rep, seed + 1, col=1)
        assert not np.array_equal(other, whole)
        v = _vectors(eng, models[1][0], 1)
    _check(flat, whole, 0, v, masks[1], models[1][0]['pi'], seed, 0, 'column 1')
    # the second column of a two-column context = a one-column context
    alone, fallen, _ = _sample(flat, models[1:], k, masks[1:], n_rep, seed)
    assert fallen == 0 and np.array_equal(alone, whole)
    # the library's own numbering off: the same states (rows and keys are the caller's ids)
    plain, _, _ = _sample(flat, models[1:], k, masks[1:], n_rep, seed, tune=dict(NO_HEIGHT_ORDER=1))
    assert np.array_equal(plain, whole)


def test_scenarios_need_a_marginal_pass():
    flat = _forest('zero64')
    with hip.Engine(flat, 1, 4) as eng:
        eng.set_models([_spec('F81', 4, flat)])
        with pytest.raises(hip.HipError, match='pml_sample_scenarios needs a marginal pml_bottom_up') as e:
            eng.sample_scenarios(8, 1)
        assert e.value.status == hip.PML_ERR_INVALID
        eng.set_masks(_tip_masks(flat, 4, 1)[None])
        eng.bottom_up(False)   # a joint sweep is not one
        with pytest.raises(hip.HipError, match='pml_sample_scenarios needs a marginal pml_bottom_up'):
            eng.sample_scenarios(8, 1)


# ---------------------------------------------------------------------------------------------------------------------
# the front end
# ---------------------------------------------------------------------------------------------------------------------

def _annotated(kind, n_tips=60, seed=12):
    """A fresh 60-tip tree with observed tips (and a few missing) and its model; tau > 0: no node is altered."""
    flat = FlatForest.random(n_tips, seed=seed, max_arity=3)
    roots = flat.to_tree_nodes()
    rng = np.random.default_rng(seed + 100)
    fs = ForestStats(roots)
    if kind == 'F81':
        states = np.array(['s{}'.format(i) for i in range(4)])
        model = F81Model(states=states, forest_stats=fs, sf=1.5 / fs.avg_nonzero_brlen, frequencies=rng.dirichlet(np.ones(4) * 3),
                         tau=0.01)
        used = 4
    else:
        model = JTTModel(forest_stats=fs, sf=1.0 / fs.avg_nonzero_brlen, tau=0.01)
        states = np.asarray(model.states)
        assert len(states) == len(JTT_STATES)
        used = 6
    for t in flat.tips:
        if rng.random() < 0.9:
            flat.nodes[t].add_feature('c', {states[int(rng.integers(used))]})
    model.freeze()
    return flat, roots, model


def _states_of(flat, name='c'):
    return np.stack([getattr(flat.nodes[i], name) for i in range(flat.n_nodes)])


@pytest.mark.parametrize('kind', ['F81', 'JTT'])
def test_scenarios_statistics(kind):
    """4096 scenarios: per-node state frequencies against the posterior (pooled chi-square, family-wise ALPHA), and the
    off-diagonal means of scenario_transition_counts against expected_counts (two-sided z test with the sample variance across
    repetitions, Bonferroni over the k (k - 1) entries at the same ALPHA; an entry that never occurs has no variance and is held
    to the Poisson probability of no event in n_rep scenarios instead)."""
    n_rep = 4096
    flat, roots, model = _annotated(kind)
    k = len(model.states)
    np.random.seed(5)
    assert sample_scenarios(roots, 'c', model, n_repetitions=n_rep) is roots
    s = _states_of(flat)
    assert s.shape == (flat.n_nodes, n_rep) and s.dtype == np.uint8
    counts = scenario_transition_counts(roots, 'c', k)
    flat2, roots2, model2 = _annotated(kind)
    problem = ml.ForestProblem(roots2, 'c', model2.states)
    try:
        problem.initialize_allowed_states()
        problem.bottom_up_loglikelihood(model2, is_marginal=True, alter=False)
        posterior = problem.top_down_marginals()[0]
    finally:
        problem.close()
    pvals = [q for q in (ref._pooled_chi2(np.bincount(s[n], minlength=k), n_rep * posterior[n] / posterior[n].sum())
                         for n in range(flat.n_nodes)) if q is not None]
    assert len(pvals) > flat.n_nodes // 4
    print('{}: min p of {} node tests = {:.3g}'.format(kind, len(pvals), min(pvals)))
    assert min(pvals) > ref.ALPHA / len(pvals)
    flat3, roots3, model3 = _annotated(kind)
    expected = ml.expected_counts(roots3, 'c', model3)
    mean = counts.mean(axis=0)
    se = counts.std(axis=0, ddof=1) / np.sqrt(n_rep)
    level = ref.ALPHA / (k * (k - 1))
    worst = 1.0
    for a in range(k):
        for b in range(k):
            if a == b:
                continue
            if se[a, b] > 0:
                p = 2 * stats.norm.sf(abs(mean[a, b] - expected[a, b]) / se[a, b])
            else:
                assert mean[a, b] == 0, (a, b, mean[a, b])
                p = float(np.exp(-n_rep * expected[a, b]))
            worst = min(worst, p)
            assert p > level, '{} -> {}: mean {} expected {} se {} p {}'.format(a, b, mean[a, b], expected[a, b], se[a, b], p)
    print('{}: min p of the {} transition tests = {:.3g}'.format(kind, k * (k - 1), worst))


def test_sample_scenarios_wrapper(monkeypatch):
    """np.random.seed fixes the result; a small device budget splits the call into chunks that make up the same array; the
    result is the restatement's for the seed the wrapper draws."""
    n_rep = 1000
    flat, roots, model = _annotated('F81')
    np.random.seed(21)
    sample_scenarios(roots, 'c', model, n_repetitions=n_rep)
    whole = _states_of(flat)
    flat2, roots2, model2 = _annotated('F81')
    monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(2 * flat2.n_nodes * 300))
    calls = []
    real = hip.Engine.sample_scenarios

    def spy(self, count, seed, rep_offset=0, col=0):
        calls.append((count, rep_offset))
        return real(self, count, seed, rep_offset=rep_offset, col=col)
    monkeypatch.setattr(hip.Engine, 'sample_scenarios', spy)
    np.random.seed(21)
    sample_scenarios(roots2, 'c', model2, n_repetitions=n_rep)
    assert calls == [(300, 0), (300, 300), (300, 600), (100, 900)]
    chunked = _states_of(flat2)
    assert chunked.dtype == np.uint8 and np.array_equal(chunked, whole)
    np.random.seed(22)
    flat3, roots3, model3 = _annotated('F81')
    sample_scenarios(roots3, 'c', model3, n_repetitions=64)
    assert not np.array_equal(_states_of(flat3), whole[:, :64])


def test_sample_scenarios_refuses_too_many_states():
    flat = FlatForest.balanced(3)
    roots = flat.to_tree_nodes()
    fs = ForestStats(roots)
    rng = np.random.default_rng(0)
    wide = F81Model(states=np.array(['s{}'.format(i) for i in range(513)]), forest_stats=fs, sf=1.0,
                    frequencies=rng.dirichlet(np.ones(513)))
    with pytest.raises(ValueError, match=r'513 states: the MI355X scenario sampler supports at most 512 states .*PML_ERR_UNSUPPORTED'):
        sample_scenarios(roots, 'c', wide, n_repetitions=4)
    k = 257
    r = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
    cr = CustomRatesModel(states=np.array(['s{}'.format(i) for i in range(k)]), forest_stats=fs, sf=1.0,
                          frequencies=rng.dirichlet(np.ones(k) * 3), rate_matrix=r + r.T)
    with pytest.raises(ValueError, match=r'257 states: the MI355X scenario sampler supports at most 256 states .*PML_ERR_UNSUPPORTED'):
        sample_scenarios(roots, 'c', cr, n_repetitions=4)
    with pytest.raises(ValueError, match='n_repetitions must be at least 1'):
        sample_scenarios(roots, 'c', wide, n_repetitions=0)
