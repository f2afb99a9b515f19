"""
P(t) of the wide eigen models in a window (``-m gpu``; csrc/pml_pij_window.h, pml_pij_window_set): the sweeps of a windowed
context must leave the BITS of the sweeps that keep P(t) of every branch, because every matrix is computed by the same
instructions and only its address changes.  Two engines of the same shape, one materialised and one windowed, on small ragged
forests (two trees, polytomies, zero-length internal branches), three columns with their own rate matrices, frequencies and
scaling factors, k = 33 (one LDS slice; the fused sweeps switched off so that all three sweeps read P(t)), 70 (two mask words;
the joint sweep reads P(t)) and 130 (two slices, three mask words; every sweep reads it), windows of the largest fan-out, of
three more and of the whole forest: ln L, bottom-up vectors and exponents, posteriors, arg-max tables, back-traced states and
MPPA masks compared with ``==`` -- also after a parameter change and a second (replayed, captured) marginal pass, and for a
sweep submitted with a partial set of active columns.  Against the reference: the k = 100 golden through a windowed engine,
and the oracle at k = 130.  Refusals by status code.  Through acr(): a character whose materialised batch does not fit the
planned memory runs windowed, with the bits of the unconstrained run.
"""
import os

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden, golden_spec
from oracle import pastml_oracle as orc
from pastml_amd import hip, synthetic
from pastml_amd.tree import FlatForest
from test_gpu_parity import LNL_RTOL, POST_RTOL, assert_same_scaled, random_masks, random_spec

pytestmark = pytest.mark.gpu

# k -> the switches under which the sweeps named in the module's docstring read P(t)
TUNES = {33: dict(NO_EIGEN_GEMM=1, NO_EIGEN_FUSED=1, NO_EIGEN_JOINT_VALU=1), 70: {}, 130: {}}
C = 3


def ragged_forest(n_tips, seed):
    """Two ragged trees with polytomies; a twentieth of the internal branches have length zero (internal ones only, and the
    masks below leave the internal nodes free: a matrix model's P(0) is the identity up to rounding dust, which must not be
    the whole likelihood where the oracle is compared, see test_gpu_fuzz.draw_case)."""
    grown = FlatForest.random(n_tips, seed=seed, max_arity=5, n_trees=2)
    rng = np.random.default_rng(seed)
    dist = grown.dist.copy()
    inner = np.flatnonzero((grown.n_children > 0) & (grown.parent >= 0))
    dist[rng.choice(inner, size=max(1, len(inner) // 20), replace=False)] = 0.0
    return FlatForest(grown.parent, grown.n_children, grown.first_child, dist, grown.roots)


_CASES = {}


def case(k):
    """(forest, specs, rates, second rates, masks) of the k-state case: made once."""
    if k not in _CASES:
        rng = np.random.default_rng(9000 + k)
        flat = ragged_forest({33: 380, 70: 300, 130: 200}[k], seed=k)
        assert 200 <= flat.n_tips <= 400 and int(flat.n_children.max()) >= 3 and len(flat.roots) == 2
        specs = [random_spec('EIGEN', k, rng) for _ in range(C)]
        rates = [(float(rng.uniform(0.3, 4)), float(rng.choice([0.0, 0.02])), float(rng.uniform(0.7, 1.0))) for _ in range(C)]
        second = [(r[0] * 1.37, r[1], r[2]) for r in rates]
        masks = np.stack([random_masks(flat, k, rng, missing=0.1, multi=0.1, internal=0.0) for _ in range(C)])
        _CASES[k] = (flat, specs, rates, second, masks)
    return _CASES[k]


def everything(k, window):
    """Every result of the case's sweeps as raw arrays; window: None (materialised) or the branches of the window."""
    flat, specs, rates, second, masks = case(k)
    out = {}
    with hip.Engine(flat, C, k, tune=TUNES[k]) as eng:
        eng.set_models(list(zip(specs, rates)))
        eng.set_masks(masks)
        if window is not None:
            eng.pij_window_set(window)
            assert eng.pij_window_info()[0] == min(window, flat.n_nodes)
        out['lnl'] = eng.bottom_up(True)
        out['bu'] = np.stack([eng.download(hip.BUF_BU, c) for c in range(C)])
        out['bu_sf'] = np.stack([eng.download(hip.BUF_BU_SF, c) for c in range(C)])
        out['post'], out['lh_sum'], out['lh_sf'] = eng.top_down_marginals()
        out['lnl_joint'] = eng.bottom_up(False)
        # (a root has no branch and no arg-max row: the sweep never writes it)
        out['tables'] = np.stack([eng.download(hip.BUF_JOINT_TABLE, c) for c in range(C)])[:, flat.parent >= 0]
        out['states'] = eng.joint_backtrace()
        out['pass_lnl'], out['pass_post'], out['pass_lh_sum'], out['pass_lh_sf'] = eng.marginal_pass()
        out['mppa'], out['mppa_n'] = eng.select_states('MPPA', force_joint=True)
        # other parameters, the masks as they were, and the pass again: the captured sweeps are replayed
        eng.set_masks(masks)
        eng.set_models(list(zip(specs, second)))
        out['second_lnl'], out['second_post'], out['second_lh_sum'], out['second_lh_sf'] = eng.marginal_pass()
        out['second_bu'] = np.stack([eng.download(hip.BUF_BU, c) for c in range(C)])
        # a sweep submitted for some of the columns.  (Only the F81 marginal kernels look at the flags: pml_bottom_up_submit_columns
        # drops them for every other sweep, so on these engines all columns are computed, by the windowed sequence as by the
        # materialised one -- what is compared is that the entry point goes through the window like the others.)
        eng.set_models(list(zip(specs, rates)))
        eng.bottom_up_submit(True, active=np.array([1, 0, 1], dtype=np.uint8))
        out['partial_lnl'] = eng.bottom_up_collect(True)
        out['partial_bu'] = np.stack([eng.download(hip.BUF_BU, c) for c in range(C)])
        eng.bottom_up_submit(False, active=np.array([0, 1, 1], dtype=np.uint8))
        out['partial_lnl_joint'] = eng.bottom_up_collect(False)
        out['info'] = eng.pij_window_info()
    return out


_MATERIALISED = {}


def materialised(k):
    if k not in _MATERIALISED:
        _MATERIALISED[k] = everything(k, None)
    return _MATERIALISED[k]


@pytest.mark.parametrize('which', ['fanout', 'fanout+3', 'nodes'])
@pytest.mark.parametrize('k', [33, 70, 130])
def test_windowed_sweeps_leave_the_bits_of_the_materialised_ones(k, which):
    flat = case(k)[0]
    fan = int(flat.n_children.max())
    window = {'fanout': fan, 'fanout+3': fan + 3, 'nodes': flat.n_nodes}[which]
    want, got = materialised(k), everything(k, window)
    assert want['info'][0] == 0 and want['info'][1] == 0 and want['info'][2] > 0     # the batch, no window
    per_branch = want['info'][2] // flat.n_nodes                                      # C k ks doubles
    assert got['info'] == (window, window * per_branch, 0)                            # the window, and the batch never was
    for name in sorted(want):
        if name == 'info':
            continue
        assert want[name].dtype == got[name].dtype and want[name].shape == got[name].shape, name
        assert np.array_equal(want[name], got[name], equal_nan=True), name
    assert np.all(np.isfinite(want['lnl'])) and np.all(np.isfinite(want['second_lnl']))
    assert not np.array_equal(want['lnl'], want['second_lnl'])                        # (the second pass did compute something else)


def test_windowed_k130_against_the_oracle():
    """The seeded k = 130 forest through a window of a few branches against the oracle, at the fuzz test's tolerances."""
    from test_gpu_fuzz import compare_vectors
    k = 130
    flat, specs, rates, _, masks = case(k)
    got = everything(k, int(flat.n_children.max()) + 3)
    internal = ~flat.is_tip
    for c in range(C):
        r = orc.full_marginal_pass(flat, masks[c].astype(int), specs[c], *rates[c])
        np.testing.assert_allclose(got['lnl'][c], r['loglik'], rtol=LNL_RTOL, atol=1e-11)
        compare_vectors(got['bu'][c], got['bu_sf'][c], r['bu'], r['bu_sf'], internal, 'BU col {}'.format(c))
        np.testing.assert_allclose(got['post'][c], r['posterior'], rtol=1e-8, atol=1e-300)
        tot = np.log10(got['lh_sum'][c]) - got['lh_sf'][c]
        np.testing.assert_allclose(tot, r['loglik_per_tree'][flat.tree_id] / np.log(10), rtol=1e-10, atol=1e-11)
        j = orc.bottom_up(flat, masks[c].astype(int), specs[c], *rates[c], is_marginal=False)
        np.testing.assert_allclose(got['lnl_joint'][c], j['loglik'], rtol=LNL_RTOL, atol=1e-11)
        # P(t) of the matrix models differs from numpy's in the last bits: a flip only between equal products
        nonroot = np.flatnonzero(flat.parent >= 0)
        for q, i in np.argwhere(got['tables'][c] != j['joint_table'][nonroot]):
            n = nonroot[q]
            prod = orc.pij(specs[c], flat.dist[n], *rates[c])[i] * j['bu'][n]
            assert abs(prod[got['tables'][c][q, i]] - prod.max()) <= 1e-12 * max(prod.max(), 1e-300), (n, i)


def test_windowed_k100_matches_the_reference():
    """The reference's own run (tests/golden/synthetic_cr_k100_L11.npz, as test_gpu_parity reads it) through a windowed engine:
    the joint sweep reads the window; the sum sweeps too where they are not fused."""
    z = load_golden('synthetic_cr_k100_L11')
    k = 100
    flat = synthetic.balanced_forest(int(z['n_levels']))
    masks = synthetic.one_hot_masks(flat, k, z['tip_states'])
    masks[np.asarray(flat.tips)[~z['tip_observed']]] = 1
    spec, rates = golden_spec(z)
    s = z['sample']
    for tune in ({}, dict(NO_EIGEN_GEMM=1)):
        with hip.Engine(flat, 1, k, tune=tune) as eng:
            eng.set_models([(spec, rates)])
            eng.set_masks(masks[None])
            eng.pij_window_set(64)
            lnl = eng.bottom_up(True)
            np.testing.assert_allclose(lnl[0], z['loglik'], rtol=LNL_RTOL)
            assert_same_scaled(eng.download(hip.BUF_BU)[s], eng.download(hip.BUF_BU_SF)[s], z['bu'], z['bu_sf'][s], what='BU')
            post, lh_sum, lh_sf = eng.top_down_marginals()
            np.testing.assert_allclose(post[0][s], z['posterior'], rtol=POST_RTOL, atol=1e-300)
            np.testing.assert_allclose(np.log10(lh_sum[0]) - lh_sf[0], lnl[0] / np.log(10), rtol=1e-11)
            lnl_j = eng.bottom_up(False)
            np.testing.assert_allclose(lnl_j[0], z['loglik_joint'], rtol=LNL_RTOL)
            table = eng.download(hip.BUF_JOINT_TABLE)[s]
            # (the reference's P(t) is numpy's product; arg-max rows may differ where two products agree to rounding)
            assert len(np.argwhere((table != z['joint_table']) & (flat.parent[s] >= 0)[:, None])) <= 2
            assert np.array_equal(eng.joint_backtrace()[0], z['joint_state'])
            assert eng.pij_window_info() == (64, 64 * k * k * 8, 0)


def test_window_refusals():
    """By status code: an F81 context, an eigen model of 20 states, a context whose P(t) is not built on the matrix cores, a
    window below the largest fan-out (the message names it), a context without a model; 0 is always accepted."""
    flat = case(70)[0]
    fan = int(flat.n_children.max())
    rng = np.random.default_rng(1)
    with hip.Engine(flat, 1, 40) as eng:
        eng.set_models([(random_spec('F81', 40, rng), (1.0, 0.0, 1.0))])
        with pytest.raises(hip.HipError) as e:
            eng.pij_window_set(flat.n_nodes)
        assert e.value.status == hip.PML_ERR_UNSUPPORTED
        eng.pij_window_set(0)
        assert eng.pij_window_info() == (0, 0, 0)
    with hip.Engine(flat, 1, 20) as eng:
        eng.set_models([(random_spec('EIGEN', 20, rng), (1.0, 0.0, 1.0))])
        with pytest.raises(hip.HipError) as e:
            eng.pij_window_set(flat.n_nodes)
        assert e.value.status == hip.PML_ERR_UNSUPPORTED
    # (the batch built by the one-thread-per-entry kernel has other bits than the matrix-core kernel the window is built with)
    with hip.Engine(flat, 1, 70, tune=dict(NO_PIJ_WIDE=1)) as eng:
        eng.set_models([(random_spec('EIGEN', 70, rng), (1.0, 0.0, 1.0))])
        with pytest.raises(hip.HipError) as e:
            eng.pij_window_set(flat.n_nodes)
        assert e.value.status == hip.PML_ERR_UNSUPPORTED
    with hip.Engine(flat, 1, 70) as eng:
        with pytest.raises(hip.HipError) as e:
            eng.pij_window_set(flat.n_nodes)            # no model yet: the kind of the context is not known
        assert e.value.status == hip.PML_ERR_INVALID
        eng.set_models([(random_spec('EIGEN', 70, rng), (1.0, 0.0, 1.0))])
        with pytest.raises(hip.HipError) as e:
            eng.pij_window_set(fan - 1)
        assert e.value.status == hip.PML_ERR_INVALID and str(fan) in str(e.value)
        with pytest.raises(hip.HipError) as e:
            eng.pij_window_set(-1)
        assert e.value.status == hip.PML_ERR_INVALID
        eng.pij_window_set(fan)
        assert eng.pij_window_info()[0] == fan
        eng.pij_window_set(0)
        assert eng.pij_window_info()[:2] == (0, 0)


def test_window_tunable_and_the_entries_that_read_the_whole_tree():
    """PASTML_HIP_PIJ_WINDOW as a per-context switch gives the window's bits too; pml_pij_batch on a windowed context still
    hands out P(t) of the whole tree (it allocates the batch for it) and the sweeps go on reading the window."""
    k = 70
    flat, specs, rates, _, masks = case(k)
    want = materialised(k)
    with hip.Engine(flat, C, k, tune=dict(PIJ_WINDOW=1)) as eng:      # (below the fan-out: raised to it)
        eng.set_models(list(zip(specs, rates)))
        eng.set_masks(masks)
        assert np.array_equal(eng.bottom_up(False), want['lnl_joint'])
        assert eng.pij_window_info()[0] == int(flat.n_children.max()) and eng.pij_window_info()[2] == 0
        with hip.Engine(flat, C, k) as plain:
            plain.set_models(list(zip(specs, rates)))
            batch = plain.pij_batch(copy_out=True)
        assert np.array_equal(eng.pij_batch(copy_out=True), batch)
        assert eng.pij_window_info()[2] > 0
        assert np.array_equal(eng.bottom_up(False), want['lnl_joint'])
        assert np.array_equal(eng.joint_backtrace(), want['states'])


def test_acr_runs_windowed_when_the_batch_does_not_fit(tmp_path, monkeypatch):
    """acr() with a CUSTOM_RATES character of more than 128 states, MPPA, and less planned memory than one materialised column
    needs: run_tasks plans a window, and the results are those of the same call with PASTML_AMD_PIJ_WINDOW=0 -- states exactly,
    ln L and parameters bit for bit (the optimiser's iterates depend on nothing but the sweeps' bits)."""
    from pastml_amd import batch as B
    from pastml_amd.acr import acr
    from pastml_amd.ml import MPPA, LOG_LIKELIHOOD, MARGINAL_PROBABILITIES, MODEL, RESTRICTED_LOG_LIKELIHOOD_FORMAT_STR
    from pastml_amd.models._eigen import save_matrix
    from pastml_amd.models.CustomRatesModel import CUSTOM_RATES
    rng = np.random.default_rng(130130)
    flat = FlatForest.random(500, seed=131, max_arity=4, lo=0.02, hi=0.4)
    flat.to_tree_nodes()   # (names the nodes as every tree made from this forest below names them)
    names = synthetic.state_names(150)
    st = np.zeros(flat.n_nodes, dtype=np.int64)
    for n in range(flat.n_nodes):   # ids are in level order: parents first
        p = flat.parent[n]
        st[n] = rng.integers(150) if p < 0 or rng.random() > np.exp(-6.0 * flat.dist[n]) else st[p]
    tips = [flat.nodes[t] for t in flat.tips]
    df = pd.DataFrame({'c': [names[st[t]] for t in flat.tips]}, index=[t.name for t in tips])
    states = np.array(sorted(set(df['c'])))
    kk = len(states)
    assert 128 < kk <= 150
    rates = np.triu(rng.uniform(0.2, 2.0, size=(kk, kk)), 1)
    rate_file = str(tmp_path / 'rates.txt')
    save_matrix(states, rates + rates.T, rate_file)
    params = {s: f for s, f in zip(states, rng.dirichlet(np.ones(kk) * 5))}
    # less than one materialised column takes, whatever its optimiser block (0.6 of it is planned)
    monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(int(B._column_bytes(flat, kk, [0], kind=hip.KIND_EIGEN))))

    def run(setting):
        hip.drain_engine_pool()
        if setting is None:
            monkeypatch.delenv('PASTML_AMD_PIJ_WINDOW', raising=False)
        else:
            monkeypatch.setenv('PASTML_AMD_PIJ_WINDOW', setting)
        t = flat.to_tree_nodes()[0]
        res = acr(t, df, prediction_method=MPPA, model=CUSTOM_RATES, column2rates={'c': rate_file}, column2parameters={'c': params})[0]
        return t, res, B.run_tasks.last_stats['pij_window']

    try:
        (ta, a, sa), (tb, b, sb) = run(None), run('0')
    finally:
        hip.drain_engine_pool()
    assert len(sa) == 1 and sa[0]['mode'] == 'windowed' and sa[0]['k'] == kk
    assert int(flat.n_children.max()) <= sa[0]['branches'] < flat.n_nodes
    assert len(sb) == 1 and sb[0]['mode'] == 'materialised' and sb[0]['branches'] == 0
    assert len({getattr(n, 'c_JOINT_STATE') for n in ta.traverse()}) > 100   # (the tips did get their states)
    assert np.isfinite(a[LOG_LIKELIHOOD]) and a[LOG_LIKELIHOOD] < -100
    assert a[LOG_LIKELIHOOD] == b[LOG_LIKELIHOOD] and a[MODEL].sf == b[MODEL].sf
    np.testing.assert_array_equal(a[MODEL].frequencies, b[MODEL].frequencies)
    key = RESTRICTED_LOG_LIKELIHOOD_FORMAT_STR.format(MPPA)
    assert a[key] == b[key] and a['num_unresolved_nodes'] == b['num_unresolved_nodes']
    assert np.array_equal(a[MARGINAL_PROBABILITIES].values, b[MARGINAL_PROBABILITIES].values)
    for na, nb in zip(FlatForest.from_trees([ta]).nodes, FlatForest.from_trees([tb]).nodes):
        assert getattr(na, 'c') == getattr(nb, 'c') and getattr(na, 'c_JOINT_STATE') == getattr(nb, 'c_JOINT_STATE')
