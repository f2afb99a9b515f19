"""
The device samplers draw for draw against their restatement (tests/sampler_ref.py): the forward simulator
(pml_simulate_states) and the scenario sampler of marginal_counts (pml_marginal_counts[_altered]).

The restatement reads the device's own inputs: E (BUF_BRANCH_EXP) or the P(t) batch the sampler reads (pij_batch), the
bottom-up vectors and posteriors (BUF_BU / BUF_POSTERIOR), and pi exactly as handed to set_models.  Every simulated state is
compared with the restatement conditioned on the device's parent states (a failure names one node), and the forward run
as a whole.  All of the simulator's arithmetic is reproducible, so no tolerance is allowed there.  The counts sampler forms
the F81 weights (1 - e) pi[a] + [a = b] e in one expression, which the compiler contracts into a v_fma_f64; a draw whose
scaled uniform lies within 1e-12 W of a cdf boundary may therefore flip between two adjacent states.  Such flips are
accepted (at most 2 per case) and reported; everything else must be equal.
"""
import warnings

import numpy as np
import pytest

import sampler_ref as ref
from oracle import pastml_oracle as orc
from pastml_amd import hip, ml
from pastml_amd.annotation import ForestStats
from pastml_amd.models._closed_form import EFTModel, JCModel
from pastml_amd.models._eigen import JTTModel
from pastml_amd.tree import FlatForest
from pastml_amd.utilities.state_simulator import simulate_states

pytestmark = pytest.mark.gpu

MAX_FLIPS = 2


# ---------------------------------------------------------------------------------------------------------------------
# forests and models
# ---------------------------------------------------------------------------------------------------------------------

def _ragged(n_tips=60, seed=3, zero_frac=0.15):
    """Several trees, polytomies, zero branches."""
    return FlatForest.random(n_tips, seed=seed, max_arity=4, zero_frac=zero_frac, n_trees=3)


def _star(n_tips, seed=1):
    """One root with n_tips tips: n_tips nodes at depth 1."""
    n = n_tips + 1
    parent = np.zeros(n, dtype=np.int32)
    parent[0] = -1
    n_children = np.zeros(n, dtype=np.int32)
    n_children[0] = n_tips
    first_child = np.zeros(n, dtype=np.int32)
    first_child[0] = 1
    dist = np.random.default_rng(seed).uniform(0.01, 0.3, size=n)
    dist[0] = 0.0
    return FlatForest(parent, n_children, first_child, dist, np.array([0]))


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


def _cherries(n, seed=7):
    """n trees of a root and two tips: n roots, n parents at depth 0."""
    N = 3 * n
    parent = np.full(N, -1, dtype=np.int32)
    parent[n:] = np.repeat(np.arange(n, dtype=np.int32), 2)
    n_children = np.zeros(N, dtype=np.int32)
    n_children[:n] = 2
    first_child = np.zeros(N, dtype=np.int32)
    first_child[:n] = n + 2 * np.arange(n)
    dist = np.random.default_rng(seed).uniform(0.01, 0.4, size=N)
    dist[:n] = 0.0
    return FlatForest(parent, n_children, first_child, dist, np.arange(n))


def _spec(kind, k, seed=0, sf=1.3, tau=0.0, flat=None):
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
    fs = ForestStats(flat.to_tree_nodes())
    states = np.array(['s{}'.format(i) for i in range(k)])
    if kind == 'JC':
        m = JCModel(states=states, forest_stats=fs, sf=sf, tau=tau)
    elif kind == 'EFT':
        m = EFTModel(states=states, forest_stats=fs, observed_frequencies=rng.dirichlet(np.ones(k) * 2), sf=sf, tau=tau)
    elif kind == 'JTT':
        m = JTTModel(forest_stats=fs, sf=sf, tau=tau)
    else:
        raise ValueError(kind)
    return m.kernel_spec(), m.rate_params()


def _device_inputs(eng, spec, col):
    """E of the column (F81 family) or the P(t) batch the sampler reads (P[n][a][b] = P_n(a -> b))."""
    if spec['kind'] == hip.KIND_F81:
        return dict(E=eng.download(hip.BUF_BRANCH_EXP, col))
    return dict(P=eng.pij_batch(copy_out=True)[col])


# ---------------------------------------------------------------------------------------------------------------------
# the simulator
# ---------------------------------------------------------------------------------------------------------------------

def _assert_sim_equal(flat, dev, spec, inputs, seed, rep_offset, label):
    n_rep = dev.shape[1]
    pi = spec['pi']
    cond = ref.simulate(flat, pi, seed, n_rep, rep_offset, parent_states=dev, **inputs)
    bad = np.argwhere(cond != dev)
    assert len(bad) == 0, '{}: {} states differ from the restatement given the device parents; first (node, rep, device, ' \
                          'restated): {}'.format(label, len(bad), [(int(n), int(r), int(dev[n, r]), int(cond[n, r]))
                                                                  for n, r in bad[:8]])
    fwd = ref.simulate(flat, pi, seed, n_rep, rep_offset, **inputs)
    assert np.array_equal(fwd, dev), label


def _simulate(flat, models, k, n_rep, seed, col=0, rep_offset=0, tune=None):
    with hip.Engine(flat, len(models), k, tune=tune) as eng:
        eng.set_models(models)
        dev = eng.simulate_states(n_rep, seed, col=col, rep_offset=rep_offset)
        inputs = _device_inputs(eng, models[col][0], col)
    assert dev.dtype == (np.uint8 if k <= 256 else np.uint16)
    return dev, inputs


def _sim_case(flat, kind, k, n_rep, seed, rep_offset=0, tau=0.1):
    models = [_spec(kind, k, tau=tau, flat=flat)]
    k = len(models[0][0]['pi'])
    dev, inputs = _simulate(flat, models, k, n_rep, seed, rep_offset=rep_offset)
    _assert_sim_equal(flat, dev, models[0][0], inputs, seed, rep_offset, '{} k={}'.format(kind, k))


SIM_MODELS = [('F81', 2), ('F81', 5), ('F81', 64), ('F81', 65), ('F81', 256), ('F81', 257), ('F81', 512), ('JC', 4),
              ('EFT', 6), ('HKY', 4), ('JTT', 20), ('CR', 7), ('CR', 33), ('CR', 100), ('CR', 128), ('CR', 129)]


@pytest.mark.parametrize('kind,k', SIM_MODELS, ids=['{}-k{}'.format(*c) for c in SIM_MODELS])
def test_simulate_models_exact(kind, k):
    """Every model family and the storage / cumulative-row paths: uint8 up to 256 states, uint16 beyond; matrix rows in LDS
    up to 128 states, in the scratch buffer beyond; a seed with a high word, an offset that is not a multiple of 4."""
    _sim_case(_ragged(), kind, k, 37, (5 << 32) + 77 + k, rep_offset=3)


@pytest.mark.parametrize('k,n_tips', [(200, 450), (256, 300)])
def test_simulate_scratch_grid_strides(k, n_tips):
    """Beyond 128 states the grid is bounded by the scratch buffer (256 MiB / (k^2 8 B): 838 workgroups at 200 states, 512 at
    256).  1025 repetitions make 2 tiles, so the depth-1 launch of a star of n_tips has 2 n_tips items, more than the grid:
    workgroups stride over items and rebuild their rows."""
    _sim_case(_star(n_tips), 'CR', k, 1025, 99 + k, tau=0.0)


def test_simulate_repetitions_offsets_and_seeds():
    """Tuple tails (1, 3, 4, 5), several tiles (1023, 1025, 4097) at every offset class (0 .. 3 mod 4, 301, 2^30 + 3), and
    seeds below and at or above 2^32."""
    flat = FlatForest.random(12, seed=9, max_arity=3, n_trees=2)
    models = [_spec('F81', 5, tau=0.05)]
    with hip.Engine(flat, 1, 5) as eng:
        eng.set_models(models)
        inputs = _device_inputs(eng, models[0][0], 0)
        for seed in (12345, (1 << 32) + 12345, (1 << 62) + 3):
            for n_rep in (1, 3, 4, 5, 1023, 1025, 4097):
                for off in (0, 1, 2, 3, 301, (1 << 30) + 3):
                    dev = eng.simulate_states(n_rep, seed, rep_offset=off)
                    _assert_sim_equal(flat, dev, models[0][0], inputs, seed, off,
                                      'seed {} n_rep {} offset {}'.format(seed, n_rep, off))


FORESTS = ['tiny', 'balanced12', 'caterpillar3000', 'ragged']


def _forest(name):
    if name == 'tiny':
        return FlatForest.balanced(2)           # level launches only
    if name == 'balanced12':
        return FlatForest.balanced(12)          # frontier inside the tree
    if name == 'caterpillar3000':
        return _caterpillar(3000)               # frontier at its cap of 16 levels
    return _ragged(zero_frac=0.2)               # several trees, polytomies, zero branches (tau > 0)


@pytest.mark.parametrize('name', FORESTS)
@pytest.mark.parametrize('kind,k', [('F81', 4), ('CR', 7)])
def test_simulate_schedules_exact(name, kind, k):
    flat = _forest(name)
    _sim_case(flat, kind, k, 40 if name != 'tiny' else 300, 4242, rep_offset=1, tau=0.05 if name == 'ragged' else 0.0)


@pytest.mark.parametrize('kind,k', [('F81', 6), ('CR', 7)])
def test_simulate_column_and_numbering(kind, k):
    """Column 1 of a 3-column engine with other parameters than column 0; the library's own numbering off gives the same
    states (the draws are keyed by the caller's ids)."""
    flat = _ragged()
    models = [_spec(kind, k, seed=c, sf=0.8 + 0.5 * c, tau=0.02 * c) for c in range(3)]
    dev, inputs = _simulate(flat, models, k, 61, 31337, col=1, rep_offset=2)
    _assert_sim_equal(flat, dev, models[1][0], inputs, 31337, 2, 'column 1')
    plain, _ = _simulate(flat, models, k, 61, 31337, col=1, rep_offset=2, tune=dict(NO_HEIGHT_ORDER=1))
    assert np.array_equal(plain, dev)


def test_simulate_states_wrapper_in_chunks(monkeypatch):
    """simulate_states() split into several device calls by a small device budget equals the restatement with the seed it
    draws from numpy."""
    flat = _ragged()
    roots = flat.to_tree_nodes()
    k = 5
    model = JCModel(states=np.array(['s{}'.format(i) for i in range(k)]), forest_stats=ForestStats(roots), sf=1.5, tau=0.1)
    n_rep = 1000
    monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(2 * flat.n_nodes * 300))
    np.random.seed(21)
    simulate_states(roots, model, 'sim', n_repetitions=n_rep)
    np.random.seed(21)
    seed = int(np.random.randint(0, 2 ** 62, dtype=np.int64))
    sim = np.stack([flat.nodes[i].sim for i in range(flat.n_nodes)])
    spec = model.kernel_spec()
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([model])
        inputs = _device_inputs(eng, spec, 0)
    _assert_sim_equal(flat, sim, spec, inputs, seed, 0, 'simulate_states')


# ---------------------------------------------------------------------------------------------------------------------
# the counts sampler
# ---------------------------------------------------------------------------------------------------------------------

def _masks(flat, k, seed, restrict_internal=True):
    """Tips observed, missing (all states) or ambiguous (2-3 states); some internal nodes restricted to half the states."""
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
    if restrict_internal and k > 2:
        internal = np.flatnonzero(flat.n_children > 0)
        for n in internal[rng.random(len(internal)) < 0.2]:
            m[n] = 0
            m[n, rng.choice(k, size=k // 2, replace=False)] = 1
    return m


def _check_counts(flat, dev, r, label):
    """Device counts / sums / same-state draws against the restatement; flips of a near-boundary draw between adjacent
    states are accepted and returned."""
    diff = dev['counts'].astype(np.int64) - r['counts']
    flips = []
    near = {}
    for n, a, b in r['near']:
        near.setdefault(n, []).append((a, b))
    for n in np.flatnonzero(np.any(diff != 0, axis=1)):
        for a, b in near.get(int(n), []):
            for nb in (b - 1, b + 1):
                if 0 <= nb < diff.shape[1] and diff[n, b] < 0 and diff[n, nb] > 0:
                    diff[n, b] += 1
                    diff[n, nb] -= 1
                    flips.append((int(n), a, b, nb))
                    break
    bad = np.flatnonzero(np.any(diff != 0, axis=1))
    assert len(bad) == 0, '{}: {} nodes differ beyond near-boundary flips; first (node, device, restated): {}; flips {}' \
        .format(label, len(bad), [(int(n), dev['counts'][n].tolist(), r['counts'][n].tolist()) for n in bad[:4]], flips)
    assert len(flips) <= MAX_FLIPS, '{}: {} near-boundary flips: {}'.format(label, len(flips), flips)
    dsum = np.abs(dev['sums'].astype(np.int64) - r['sums']).sum()
    assert dsum <= 3 * len(flips), '{}: sums differ by {} (flips {})'.format(label, dsum, flips)
    dsame = np.abs(dev['same'].astype(np.int64) - r['same']).sum()
    assert dsame <= 2 * len(flips), '{}: same-state draws differ by {} (flips {})'.format(label, dsame, flips)
    if flips:
        warnings.warn('{}: accepted near-boundary flips (node, parent state, restated, device): {}'.format(label, flips))
    return flips


def _counts_case(flat, models, k, masks, n_rep, seed, col=0, tune=None):
    """marginal_counts_altered with nothing altered on column col, checked against the restatement conditioned on the
    device's parent counts; pml_marginal_counts with the same seed gives the sums / n_rep.  Returns the device's counts."""
    with hip.Engine(flat, len(models), k, tune=tune) as eng:
        eng.set_models(models)
        eng.set_masks(masks)
        eng.bottom_up(True)
        eng.top_down_marginals()
        sums, cnt, same = eng.marginal_counts_altered(n_rep, seed, np.zeros(flat.n_nodes, dtype=np.uint8), col=col)
        plain = eng.marginal_counts(n_rep, seed, col=col)
        bu = eng.download(hip.BUF_BU, col)
        post = eng.download(hip.BUF_POSTERIOR, col)
        inputs = _device_inputs(eng, models[col][0], col)
    assert np.array_equal(plain, sums / n_rep)
    assert np.all(cnt.sum(axis=1) == n_rep)
    r = ref.counts(flat, masks[col], bu, post, models[col][0]['pi'], seed, n_rep, parent_counts=cnt, **inputs)
    _check_counts(flat, dict(counts=cnt, sums=sums, same=same), r, 'k={} n_rep={} col={}'.format(k, n_rep, col))
    return cnt, sums


def _counts_forest():
    return FlatForest.random(50, seed=11, max_arity=4, n_trees=2)


COUNT_MODELS = [('F81', 2), ('F81', 4), ('F81', 63), ('F81', 64), ('F81', 65), ('F81', 130), ('F81', 256), ('HKY', 4),
                ('JTT', 20), ('CR', 100), ('CR', 200)]


@pytest.mark.parametrize('kind,k', COUNT_MODELS, ids=['{}-k{}'.format(*c) for c in COUNT_MODELS])
def test_counts_models_exact(kind, k):
    flat = _counts_forest()
    models = [_spec(kind, k, sf=1.1, flat=flat)]
    k = len(models[0][0]['pi'])
    masks = _masks(flat, k, k)[None]
    _counts_case(flat, models, k, masks, 200, (3 << 32) + k)


@pytest.mark.parametrize('n_rep', [1, 63, 64, 65, 1000])
def test_counts_repetitions_exact(n_rep):
    flat = _counts_forest()
    models = [_spec('F81', 5, sf=1.1)]
    _counts_case(flat, models, 5, _masks(flat, 5, 1)[None], n_rep, 777 + n_rep)


def test_counts_many_roots_and_parents():
    """70 000 cherries: more than 1 024 roots (the roots kernel's grid) and more than 65 536 parents at one depth (the
    level kernel's grid): both stride."""
    flat = _cherries(70000)
    k = 4
    _counts_case(flat, [_spec('F81', k, sf=1.0)], k, _masks(flat, k, 3, restrict_internal=False)[None], 16, 5)


@pytest.mark.parametrize('kind,k', [('F81', 6), ('HKY', 4)])
def test_counts_column_and_numbering(kind, k):
    flat = _counts_forest()
    models = [_spec(kind, k, seed=c, sf=0.8 + 0.4 * c) for c in range(3)]
    masks = np.stack([_masks(flat, k, 40 + c) for c in range(3)])
    cnt, sums = _counts_case(flat, models, k, masks, 300, 2718, col=1)
    cnt2, sums2 = _counts_case(flat, models, k, masks, 300, 2718, col=1, tune=dict(NO_HEIGHT_ORDER=1))
    assert np.array_equal(cnt, cnt2) and np.array_equal(sums, sums2)


@pytest.mark.parametrize('kind,k', [('F81', 6), ('JTT', 20)])
def test_counts_altered_nodes_exact(kind, k):
    """Zero-branch forests through ml.marginal_counts: the device's part (counts, sums without altered pairs, same-state
    draws of the dirty parents) against the restatement, and the result against the fractional counts assembled from it."""
    from pastml_amd.models.JTTModel import JTT_STATES
    rng = np.random.default_rng(50 + k)
    flat = FlatForest.random(90, seed=23 + k, max_arity=3, zero_frac=0.3)
    roots = flat.to_tree_nodes()
    states = np.array(JTT_STATES) if kind == 'JTT' else np.array(['s{}'.format(i) for i in range(k)])
    initial = np.ones((flat.n_nodes, k), dtype=np.int8)
    for t in flat.tips:
        if rng.random() < 0.9:
            s = int(rng.integers(k))
            flat.nodes[t].add_feature('c', {states[s]})
            initial[t] = 0
            initial[t, s] = 1
    fs = ForestStats(roots)
    if kind == 'F81':
        from pastml_amd.models._closed_form import F81Model
        model = F81Model(states=states, forest_stats=fs, sf=1.2 / fs.avg_nonzero_brlen, frequencies=rng.dirichlet(np.ones(k) * 3))
    else:
        model = JTTModel(states=states, forest_stats=fs, sf=0.8 / fs.avg_nonzero_brlen)
    model.freeze()
    n_rep = 500
    seen = []
    real = hip.Engine.marginal_counts_altered

    def spy(self, n_repetitions, seed, altered, col=0):
        out = real(self, n_repetitions, seed, altered, col=col)
        assert np.array_equal(self.flat.parent, flat.parent)
        spec = model.kernel_spec()
        # (copies: the caller adds the fractional counts into the sums it was handed)
        seen.append(dict(seed=seed, altered=np.asarray(altered, dtype=bool), out=tuple(np.array(x) for x in out), bu=self.download(hip.BUF_BU, col),
                         post=self.download(hip.BUF_POSTERIOR, col), inputs=_device_inputs(self, spec, col), pi=spec['pi']))
        return out
    hip.Engine.marginal_counts_altered = spy
    try:
        np.random.seed(3)
        got = ml.marginal_counts(roots, 'c', model, n_repetitions=n_rep)
    finally:
        hip.Engine.marginal_counts_altered = real
    assert len(seen) == 1, 'no node was altered: the test does not test what it says'
    s = seen[0]
    sums, cnt, same = s['out']
    alt = s['altered']
    assert alt.any()
    tip = flat.n_children == 0
    # (an internal node's bottom-up vector carries its mask; the tips' rows of BUF_BU are their masks)
    masks = np.where(tip[:, None], s['bu'], 1.0)
    r = ref.counts(flat, masks, s['bu'], s['post'], s['pi'], s['seed'], n_rep, parent_counts=cnt, altered=alt, **s['inputs'])
    flips = _check_counts(flat, dict(counts=cnt, sums=sums, same=same), r, '{} altered'.format(kind))
    assert not flips or kind == 'F81'
    want = ref.altered_assembly(flat, sums, cnt, same, alt, initial, n_rep)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
