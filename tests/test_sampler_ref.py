"""The restatement of the device samplers' draws (tests/sampler_ref.py): Philox known answers, the scan, and that the
restated draws are the right estimators (they pass the statistical yardsticks the device is held to).  No GPU."""
import numpy as np

import sampler_ref as ref
from conftest import load_golden
from oracle import pastml_oracle as orc
from pastml_amd import synthetic
from pastml_amd.tree import FlatForest


def _hex(words):
    return ' '.join('{:08x}'.format(int(w)) for w in words)


def test_philox_known_answers():
    """Random123's known-answer vectors of Philox-4x32-10."""
    assert _hex(ref.philox4x32_10((0, 0, 0, 0), 0, 0)) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    m = 0xffffffff
    assert _hex(ref.philox4x32_10((m, m, m, m), m, m)) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    got = ref.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), 0xa4093822, 0x299f31d0)
    assert _hex(got) == 'd16cfe09 94fdcceb 5001e420 24126ea1'
    # vectorised: the same answers in any position of a batch
    batch = ref.philox4x32_10((np.array([0, m, 0x243f6a88]), np.array([0, m, 0x85a308d3]), np.array([0, m, 0x13198a2e]),
                               np.array([0, m, 0x03707344])), 0, 0)
    assert _hex(batch[:, 0]) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'


def test_uniform_mappings():
    """Simulator: word g & 3 of block g >> 2, 32 bits; counts: 53 bits of words 0 and 1."""
    seed = (7 << 32) | 12345
    w = ref.philox4x32_10((5, 9, 0, ref.SIM_TAG), 12345, 7)
    u = ref.sim_uniforms(seed, 9, np.arange(20, 24))
    assert np.array_equal(u, w.astype(np.float64) * 2.0 ** -32)
    assert np.all((u >= 0) & (u < 1))
    w = ref.philox4x32_10((3, 2, 9, ref.COUNTS_TAG), 12345, 7)
    u = ref.counts_uniforms(seed, 9, 2, 3)
    assert u == float(((int(w[0]) << 32) | int(w[1])) >> 11) * 2.0 ** -53
    # keys, states and draws are independent dimensions: no two of these collide
    us = ref.counts_uniforms(seed, np.arange(4)[:, None, None], np.arange(4)[None, :, None], np.arange(4)[None, None, :])
    assert len(np.unique(us)) == 64
    us = ref.sim_uniforms(seed, np.arange(8)[:, None], np.arange(64)[None, :])
    assert len(np.unique(us)) == 8 * 64


def test_wave_scan_is_a_sum():
    rng = np.random.default_rng(0)
    for k in (1, 63, 64, 65, 200):
        x = rng.dirichlet(np.ones(k)) * rng.uniform(0.1, 10)
        x[rng.random(k) < 0.2] = 0.0
        inc, total = ref.wave_scan(x)
        cs = np.cumsum(x)
        np.testing.assert_allclose(inc, cs, rtol=8 * np.finfo(float).eps, atol=0)
        assert abs(total - cs[-1]) <= 8 * np.finfo(float).eps * cs[-1]
        # batched rows scan independently
        inc2, total2 = ref.wave_scan(np.stack([x, 2 * x]))
        assert np.array_equal(inc2[0], inc) and np.array_equal(inc2[1], 2 * inc) and total2[0] == total


def test_bisect_first_greater():
    cdf = np.array([[0.0, 0.25, 0.25, 0.5, 1.0]])
    w = np.array([0.0, 0.1, 0.25, 0.3, 0.5, 0.99, 1.0])
    assert list(ref.bisect(cdf, np.zeros(len(w), dtype=np.int64), w)) == [1, 1, 3, 3, 4, 4, 4]


def _sim_forest():
    return FlatForest.random(40, seed=3, max_arity=4, zero_frac=0.15, n_trees=3)


class _OracleModel(object):
    """What _check_transitions reads of a model (frequencies, get_Pij_t), from the oracle's P(t)."""

    def __init__(self, spec, sf, tau):
        self.spec, self.sf, self.tau = spec, sf, tau
        self.frequencies = spec['pi']

    def get_Pij_t(self, t):
        return orc.pij(self.spec, t, self.sf, self.tau)


def test_restated_simulation_passes_the_transition_test():
    """The restated simulator is a sampler of P(t): the per-branch chi-square of the device's statistical tests."""
    flat = _sim_forest()
    rng = np.random.default_rng(5)
    k = 5
    f81 = _OracleModel(dict(kind=orc.KIND_F81, pi=rng.dirichlet(np.ones(k) * 2)), 1.7, 0.1)
    P = np.stack([f81.get_Pij_t(float(t)) for t in flat.dist])
    E = P[:, 0, 0] - P[:, 1, 0]   # P_aa - P_ba = e
    sim = ref.simulate(flat, f81.frequencies, 99, 4000, E=E)
    ref._check_transitions(flat, f81, sim, k)
    k = 6
    rates = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
    pi = rng.dirichlet(np.ones(k) * 3)
    d, a, ainv = orc.diagonalise(pi, rates + rates.T)
    cr = _OracleModel(dict(kind=orc.KIND_EIGEN, pi=pi, d=d, A=a, Ainv=ainv), 1.7, 0.0)
    P = np.stack([cr.get_Pij_t(float(t)) for t in flat.dist])
    sim = ref.simulate(flat, pi, (1 << 40) + 3, 4000, rep_offset=7, P=P)
    ref._check_transitions(flat, cr, sim, k)
    # conditioning on the restated parents' states reproduces the forward run
    assert np.array_equal(ref.simulate(flat, pi, (1 << 40) + 3, 4000, rep_offset=7, P=P, parent_states=sim), sim)
    # chunks of repetitions make up the whole
    parts = np.concatenate([ref.simulate(flat, pi, 5, 301, P=P), ref.simulate(flat, pi, 5, 99, rep_offset=301, P=P)], axis=1)
    assert np.array_equal(parts, ref.simulate(flat, pi, 5, 400, P=P))


def test_restated_counts_agree_with_the_reference_estimate():
    """The restated scenario sampler on the oracle's bottom-up vectors and posteriors against the reference's own
    marginal_counts estimate (tests/golden/marginal_counts.npz, JC on 64 tips), with the tolerance of
    test_marginal_counts_statistical_parity."""
    z = load_golden('marginal_counts')
    n_rep = int(z['n_repetitions'])
    flat = synthetic.balanced_forest(6)
    k = 4
    masks = np.ones((flat.n_nodes, k), dtype=int)
    masks[flat.tips] = 0
    masks[flat.tips, z['jc_tip_states']] = 1
    spec = dict(kind=orc.KIND_F81, pi=np.full(k, 0.25))
    sf = float(z['jc_sf'])
    r = orc.full_marginal_pass(flat, masks, spec, sf=sf)
    P = np.stack([orc.pij(spec, float(t), sf) for t in flat.dist])
    E = P[:, 0, 0] - P[:, 1, 0]
    out = ref.counts(flat, masks, r['bu'], r['posterior'], spec['pi'], 2024, n_rep, E=E)
    assert out['counts'].sum(axis=1).tolist() == [n_rep] * flat.n_nodes
    ours = out['sums'] / n_rep
    want = z['jc_counts']
    tol = 6 * np.sqrt(np.maximum(want, 0.05) / n_rep) * 3 + 0.02
    assert np.all(np.abs(ours - want) < tol), np.abs(ours - want).max()
    assert abs(ours.sum() - want.sum()) < 0.3
    # the same estimate through the matrix path (P[n][b][a] read instead of the F81 closed form)
    out_p = ref.counts(flat, masks, r['bu'], r['posterior'], spec['pi'], 2024, n_rep, P=P)
    assert np.all(np.abs(out_p['sums'] / n_rep - want) < tol)


def test_altered_assembly_without_altered_nodes_is_the_sums():
    flat = FlatForest.random(12, seed=1, max_arity=3)
    rng = np.random.default_rng(2)
    k = 3
    sums = rng.integers(0, 50, size=(k, k))
    cnt = rng.integers(0, 10, size=(flat.n_nodes, k))
    got = ref.altered_assembly(flat, sums, cnt, np.zeros_like(cnt), np.zeros(flat.n_nodes, dtype=bool),
                               np.ones((flat.n_nodes, k)), 10)
    assert np.array_equal(got, sums / 10)
    # an altered tip whose counts miss its initial states: spread over them; its parent's row gets the fractions
    alt = np.zeros(flat.n_nodes, dtype=bool)
    tip = int(flat.tips[0])
    p = int(flat.parent[tip])
    alt[tip] = True
    init = np.ones((flat.n_nodes, k))
    init[tip] = [0, 1, 0]
    cnt = np.zeros((flat.n_nodes, k), dtype=np.int64)
    cnt[p] = [10, 0, 0]
    cnt[tip] = [10, 0, 0]
    got = ref.altered_assembly(flat, np.zeros((k, k)), cnt, np.zeros_like(cnt), alt, init, 10)
    want = np.zeros((k, k))
    want[0, 1] = 1.0
    assert np.array_equal(got, want)

