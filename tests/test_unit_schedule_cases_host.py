"""
The columns of tests/unit_schedule_cases.py on the host: every (forest, k, parameter set, column) that
test_gpu_consumers_on_unit_schedules.py runs has a finite ln L in exact arithmetic (tests/f81_exact_ref.py) and no internal node
whose posterior row is all zero, at tau = 0 as at tau > 0 -- so the GPU file has no case to skip or to filter out.
"""
import numpy as np
import pytest

import f81_exact_ref as exact
import unit_schedule_cases as units


def test_the_cases_are_the_ones_the_issue_names():
    assert sorted(k for name, k in units.FOREST_KS if name == 'chained') == [17, 20, 32, 33, 64]
    for name in ('clumps', 'ragged'):
        assert sorted(k for n, k in units.FOREST_KS if n == name) == [20, 64]
    assert set(units.OTHER_PARAMETERS) <= set(units.FOREST_KS)
    chained, clumps, ragged = (units.forest(name) for name in ('chained', 'clumps', 'ragged'))
    assert (chained.n_nodes, len(chained.tips)) == (255, 128)
    assert clumps.n_nodes == 256 and len(clumps.roots) == 2
    assert int(((clumps.parent >= 0) & (clumps.dist == 0)).sum()) == 46
    assert int(ragged.n_children.max()) == 3
    # every case has a column at each tau, and the other parameters are other parameters at the other tau
    for name, k, p in units.USES:
        taus = [rates[1] for _, rates in units.models(name, k, p)]
        assert set(taus) == set(units.TAUS), (name, k, p)
    for name, k in units.OTHER_PARAMETERS:
        for (a, ra), (b, rb) in zip(units.models(name, k, 0), units.models(name, k, 1)):
            assert not np.array_equal(a['pi'], b['pi']) and ra[0] != rb[0] and ra[1] != rb[1]


def test_the_masks_are_of_every_kind():
    flat = units.forest('chained')
    tips, internal = np.asarray(flat.tips), np.flatnonzero(flat.n_children > 0)
    for k in (17, 64):
        m = units.masks('chained', k)
        assert m.shape == (5, flat.n_nodes, k)
        width = m.sum(axis=2)
        assert (width[1, tips] == 1).all() and (width[1, internal] == k).all()                      # observed
        assert (width[2, tips] == k).any() and set(np.unique(width[2, tips])) <= {1, k}            # unobserved
        assert ((width[3, tips] > 1) & (width[3, tips] < k)).any()                                  # ambiguous
        assert (width[4, tips] == 1).all() and (width[4, internal] < k).any()                       # restricted internal nodes
    flat = units.forest('clumps')
    zero_tips = tips = np.asarray(flat.tips)[flat.dist[flat.tips] == 0]
    assert len(zero_tips) > 0 and (units.masks('clumps', 20)[:, zero_tips] == 1).all()
    assert units.altered('clumps').sum() > 0 and units.altered('chained').sum() > 0


def test_the_bins_cut_branches_and_one_is_empty():
    for name in ('chained', 'clumps', 'ragged'):
        flat, t, b = units.forest(name), units.node_times(name), units.boundaries(name)
        assert len(b) == 6 and (np.diff(b) > 0).all()
        has = flat.parent >= 0
        cut = [int(((t[flat.parent[has]] < x) & (x < t[has])).sum()) for x in b]
        assert min(cut[1:4]) > 0 and cut[4] == cut[5] == 0, cut
        assert b[4] > t.max() and np.isin(b, t).sum() == 1


@pytest.mark.parametrize('name, k, p', units.USES)
def test_every_column_has_a_likelihood_and_posteriors(name, k, p):
    flat, masks, models = units.forest(name), units.masks(name, k), units.models(name, k, p)
    assert len(masks) == len(models) == units.N_COLUMNS[name]
    internal = np.flatnonzero(flat.n_children > 0)
    for c, (spec, (sf, tau, tf)) in enumerate(models):
        want = exact.marginal_pass(flat, masks[c], spec['pi'], sf, tau, tf, top_down=True, vectors=False)
        assert want['loglik'].is_finite(), (name, k, p, c, tau)
        post = want['posterior']
        assert np.isfinite(post).all() and (post[internal].max(axis=1) > 0).all(), (name, k, p, c, tau)
