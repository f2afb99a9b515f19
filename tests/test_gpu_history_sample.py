"""
Histories drawn on the device (pml_sample_histories, Engine.sample_histories) draw for draw against their restatement
(tests/history_sample_ref.py) conditioned on the device's own scenarios and on the exponentials the device stored
(BUF_BRANCH_EXP), on the forests of test_gpu_scenarios.py.

branch_jumps and jumps are compared exactly.  times entry by entry within (summands + 16) * 2^-52 relative: all terms are
non-negative, a dwell is three rounded operations on a log good to an ulp, and a sum of m positive terms is off by at most m
roundings.  The policy for draws at a boundary is that of test_gpu_sampler_exact.py: a repetition with a (node, repetition) pair
the restatement lists as near is left out of the times / jumps comparison and its branch_jumps may differ at that node only, at
most 2 per case; the restatement's own list has at most 2 entries for the fixed seeds.
"""
import math
import re

import numpy as np
import pytest

import history_sample_ref as hs
from pastml_amd import hip
from test_gpu_scenarios import _forest, _spec, _masks, _marginal_pass

pytestmark = pytest.mark.gpu

MAX_NEAR = 2
BOUND = 5.0   # standard errors


def _model(kind, k, flat, tree, x_top=None):
    spec, (sf, tau, tf) = _spec(kind, k, flat, tau=0.0 if tree == 'zero64' else 0.1)
    if x_top is not None:   # sf such that the longest branch has x = x_top
        mu = 1.0 / (1.0 - float(np.dot(spec['pi'], spec['pi'])))
        sf = x_top / (mu * (flat.dist[flat.parent >= 0].max() + tau) * tf)
    return spec, (sf, tau, tf)


def _draw(flat, model, k, masks, n_rep, seed, rep_offset=0, tune=None, **what):
    with hip.Engine(flat, 1, k, tune=tune) as eng:
        _marginal_pass(eng, [model], masks)
        out = eng.sample_histories(n_rep, seed, rep_offset=rep_offset, **what)
        E = eng.download(hip.BUF_BRANCH_EXP, 0)
    return out, E


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def _check(flat, out, E, model, seed, rep_offset, label):
    states, times, jumps, branch, fallen = out
    spec, (sf, tau, tf) = model
    N, n_rep = states.shape
    k = len(spec['pi'])
    assert times.shape == (n_rep, k) and times.dtype == np.float64, label
    assert jumps.shape == (n_rep, k, k) and jumps.dtype == np.uint32, label
    assert branch.shape == (N, n_rep) and branch.dtype == np.uint16, label
    assert fallen == 0, label
    r = hs.histories(flat, states, spec['pi'], E, sf, tau, tf, seed, rep_offset)
    assert r['n_skipped'] == 0, label
    assert len(r['near']) <= MAX_NEAR, '{}: the restatement lists {} near pairs: pick another seed'.format(label, len(r['near']))
    near = set(r['near'])
    keep = np.ones(n_rep, dtype=bool)
    keep[[rep for _, rep in near]] = False
    bad = [(int(n), int(q)) for n, q in np.argwhere(branch != r['branch_jumps'])]
    assert all(pair in near for pair in bad), '{}: branch_jumps differ at (node, repetition) {} (device, restated: {})'.format(
        label, bad[:8], [(int(branch[n, q]), int(r['branch_jumps'][n, q])) for n, q in bad[:8]])
    assert len(bad) <= MAX_NEAR, label
    assert np.array_equal(jumps[keep], r['jumps'][keep]), '{}: {} jumps entries differ'.format(
        label, int((jumps[keep] != r['jumps'][keep]).sum()))
    want, m = r['times'][keep], r['summands'][keep]
    got = times[keep]
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(want > 0, err / ((m + 16) * 2.0 ** -52 * want), np.where(got == 0.0, 0.0, np.inf))
    worst = float(ratio.max()) if ratio.size else 0.0
    print('{}: {} near pairs, {} branch_jumps flips; times: worst error / bound {:.3g}, most events on a branch {}'.format(
        label, len(near), len(bad), worst, int(r['events'].max()) if r['events'].size else 0))
    assert worst <= 1.0, (label, worst)
    # the identities of a history, on the device's own output
    length = ((flat.dist[flat.parent >= 0] + tau) * tf).sum()
    assert np.allclose(times.sum(axis=1), length, rtol=1e-12, atol=0), label
    assert (jumps[:, np.arange(k), np.arange(k)] == 0).all(), label
    assert np.array_equal(jumps.astype(np.int64).sum(axis=(1, 2)), branch.astype(np.int64).sum(axis=0)), label
    assert (branch[flat.parent < 0] == 0).all(), label
    return r


# (tree, kind, k, repetitions, rep_offset, x on the longest branch or None: the forests' own sf)
# Repetitions to a workgroup (hsamp_tile: the largest of 256, 128, 64 whose accumulators fit 136 KiB of LDS): 256 up to 67
# states, 128 up to 133, 64 up to 256 -- both sides of each step are cases; 65: two chunks of the pi table; 300: uint16 states
# and the accumulators in HBM.  forest300 is 8 pieces of 64 ids; 1024 repetitions: several tiles; 250, 130 and 1: a ragged tile.
CASES = [
    ('forest300', 'F81', 2, 1024, 0, None),
    ('forest300', 'F81', 4, 250, 3, None),
    ('forest300', 'F81', 4, 1, 0, None),
    ('forest300', 'JC', 4, 1024, 0, None),
    ('forest300', 'F81', 64, 250, 3, None),
    ('forest300', 'F81', 65, 1024, 0, None),
    ('forest300', 'F81', 300, 250, 3, None),
    ('forest300', 'F81', 4, 250, 5, 30.0),
    ('caterpillar200', 'F81', 4, 250, 3, None),
    ('caterpillar200', 'F81', 65, 1, 0, None),
    ('caterpillar200', 'F81', 256, 64, 0, None),
    ('caterpillar200', 'F81', 300, 1, 2, None),
    ('zero64', 'F81', 4, 250, 3, None),
    ('zero64', 'F81', 64, 1024, 0, None),
    ('zero64', 'F81', 67, 250, 0, None),
    ('zero64', 'F81', 68, 250, 1, None),
    ('zero64', 'F81', 133, 130, 0, None),
    ('zero64', 'F81', 134, 130, 2, None),
    ('single', 'F81', 4, 250, 3, None),
    ('single', 'F81', 300, 1, 0, None),
]


@pytest.mark.parametrize('tree, kind, k, n_rep, rep_offset, x_top', CASES,
                         ids=['{}-{}-k{}-r{}{}'.format(c[0], c[1], c[2], c[3], '-x30' if c[5] else '') for c in CASES])
def test_histories_draw_for_draw(tree, kind, k, n_rep, rep_offset, x_top):
    flat = _forest(tree)
    model = _model(kind, k, flat, tree, x_top)
    masks = _masks(flat, k, 7 * k + 1, tree)[None]
    seed = (9 << 32) + 1000 * k + n_rep + len(tree)
    out, E = _draw(flat, model, k, masks, n_rep, seed, rep_offset, branch_jumps=True)
    assert out[0].dtype == (np.uint8 if k <= 256 else np.uint16)
    r = _check(flat, out, E, model, seed, rep_offset, '{} {} k={} n_rep={}'.format(tree, kind, k, n_rep))
    if x_top is not None:
        assert r['events'].max() >= 30, 'no long branch in the case'
    if tree == 'zero64':
        zero = (flat.parent >= 0) & (flat.dist == 0)
        assert zero.any() and (out[3][zero] == 0).all()


def test_states_are_the_scenarios_chunks_make_up_a_call_and_outputs_are_independent():
    flat = _forest('forest300')
    k, n_rep, seed = 6, 300, 31337
    model = _model('F81', k, flat, 'forest300')
    masks = _masks(flat, k, 40)[None]
    with hip.Engine(flat, 1, k) as eng:
        _marginal_pass(eng, [model], masks)
        whole = eng.sample_histories(n_rep, seed, branch_jumps=True)
        scenarios, fallen = eng.sample_scenarios(n_rep, seed)
        assert fallen == 0 and whole[4] == 0
        assert whole[0].dtype == scenarios.dtype and np.array_equal(whole[0], scenarios)
        # calls with rep_offset 0 / 6 / 130 make up one call, bit for bit
        parts = [eng.sample_histories(c, seed, rep_offset=o, branch_jumps=True) for o, c in ((0, 6), (6, 124), (130, n_rep - 130))]
        for i, axis in enumerate((1, 0, 0, 1)):
            assert np.array_equal(np.concatenate([p[i] for p in parts], axis=axis), whole[i]), i
        assert not np.array_equal(eng.sample_histories(n_rep, seed + 1)[1], whole[1])
        # what is not asked for is not computed, and times has the same bits
        for jumps, branch_jumps, states in ((False, False, False), (False, True, True), (True, False, False)):
            got = eng.sample_histories(n_rep, seed, jumps=jumps, branch_jumps=branch_jumps, states=states)
            assert np.array_equal(got[1], whole[1])
            assert (got[0] is None) == (not states) and (got[2] is None) == (not jumps) and (got[3] is None) == (not branch_jumps)
            assert _same([x for x in got[:4] if x is not None], [y for x, y in zip(got[:4], whole[:4]) if x is not None])
        assert np.array_equal(eng.sample_scenarios(n_rep, seed)[0], scenarios)   # (the results of the pass stay)


@pytest.mark.parametrize('k', [4, 300])
def test_bits_do_not_depend_on_schedules_or_numbering(k):
    flat = _forest('forest300')
    assert flat.n_nodes > 2 * 64, 'one piece only'
    n_rep, seed = 200, 777 + k
    model = _model('F81', k, flat, 'forest300')
    masks = _masks(flat, k, 3)[None]
    base, _ = _draw(flat, model, k, masks, n_rep, seed, branch_jumps=True)
    for tune in (dict(NO_HEIGHT_ORDER=1), dict(NO_SUPER=1)):   # (the caller's numbering kept; the sweeps' other schedule)
        other, _ = _draw(flat, model, k, masks, n_rep, seed, tune=tune, branch_jumps=True)
        assert _same(base[:4], other[:4]), tune


def test_means_are_the_device_expected_history():
    flat = _forest('forest300')
    k, n_rep, seed = 4, 4096, (3 << 32) + 99
    model = _model('F81', k, flat, 'forest300', x_top=2.0)
    masks = _masks(flat, k, 29)[None]
    with hip.Engine(flat, 1, k) as eng:
        _marginal_pass(eng, [model], masks)
        exact_times, exact_jumps, _ = eng.expected_history()
        _, times, jumps, _, fallen = eng.sample_histories(n_rep, seed, states=False)
    assert fallen == 0
    n_times = n_jumps = 0
    for s in range(k):
        se = times[:, s].std(ddof=1) / math.sqrt(n_rep)
        z = abs(times[:, s].mean() - exact_times[0, s]) / se
        print('times[{}]: mean {:.6g} exact {:.6g} z {:.2f}'.format(s, times[:, s].mean(), exact_times[0, s], z))
        assert z <= BOUND, (s, z)
        n_times += 1
    for i in range(k):
        for j in range(k):
            if i == j or exact_jumps[0, i, j] < 1.0:
                continue
            col = jumps[:, i, j].astype(np.float64)
            se = col.std(ddof=1) / math.sqrt(n_rep)
            z = abs(col.mean() - exact_jumps[0, i, j]) / se
            print('jumps[{}][{}]: mean {:.6g} exact {:.6g} z {:.2f}'.format(i, j, col.mean(), exact_jumps[0, i, j], z))
            assert z <= BOUND, (i, j, z)
            n_jumps += 1
    assert n_times >= k and n_jumps >= 2, (n_times, n_jumps)


def _refused(call, status, *words):
    with pytest.raises(hip.HipError) as info:
        call()
    assert info.value.status == status, str(info.value)
    for word in words:
        assert word in str(info.value), str(info.value)
    return str(info.value)


def test_refusals_leave_the_context_answering():
    flat = _forest('zero64')
    k = 4
    masks = _masks(flat, k, 5, 'forest300')[None]
    # no marginal pass
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([_model('F81', k, flat, 'forest300')])
        eng.set_masks(masks)
        _refused(lambda: eng.sample_histories(8, 1), hip.PML_ERR_INVALID, 'pml_sample_histories needs a marginal pml_bottom_up')
        eng.bottom_up(False)   # a joint sweep is not one
        _refused(lambda: eng.sample_histories(8, 1), hip.PML_ERR_INVALID, 'pml_sample_histories needs a marginal pml_bottom_up')
    # a model kind other than F81
    with hip.Engine(flat, 1, 4) as eng:
        _marginal_pass(eng, [_spec('HKY', 4, flat)], masks)
        counts = eng.expected_counts()
        _refused(lambda: eng.sample_histories(8, 1), hip.PML_ERR_UNSUPPORTED, 'pml_sample_histories', 'F81', 'HKY')
        assert np.array_equal(eng.expected_counts(), counts)
    # branches with x > 512
    spec, (sf, tau, tf) = _model('F81', k, flat, 'forest300')
    model = (spec, (2000.0, tau, tf))
    _, x, _ = hs.branch_scalars(flat, spec['pi'], 2000.0, tau, tf)
    n_long = int((x[flat.parent >= 0] > hs.MAX_X).sum())
    assert 0 < n_long < int((flat.parent >= 0).sum())
    with hip.Engine(flat, 1, k) as eng:
        _marginal_pass(eng, [model], masks)
        counts = eng.expected_counts()
        text = _refused(lambda: eng.sample_histories(70, 1, branch_jumps=True), hip.PML_ERR_UNSUPPORTED, 'pml_sample_histories', '512')
        assert int(re.search(r'(\d+) branches', text).group(1)) == n_long, text
        assert np.array_equal(eng.expected_counts(), counts)   # (the results of the pass stay)
        assert eng.sample_scenarios(8, 1)[0].shape == (flat.n_nodes, 8)


def test_sample_histories_front_end(monkeypatch):
    """np.random.seed fixes the result; the scenarios attached are sample_scenarios' for the same seed; a small device budget
    splits the call into chunks that make up the same arrays; history_summary brackets the device's expected_history."""
    from pastml_amd import ml
    from pastml_amd.utilities.history_sampler import history_summary, sample_histories
    from pastml_amd.utilities.scenario_sampler import sample_scenarios
    from test_gpu_scenarios import _annotated, _states_of
    n_rep = 1000
    flat, roots, model = _annotated('F81')
    np.random.seed(21)
    whole = sample_histories(roots, 'c', model, n_repetitions=n_rep, branch_jumps=True)
    k = len(model.states)
    assert whole['times'].shape == (n_rep, k) and whole['jumps'].shape == (n_rep, k, k)
    assert whole['branch_jumps'].shape == (flat.n_nodes, n_rep)
    assert np.allclose(whole['times'].sum(axis=1), whole['tree_length'], rtol=1e-12, atol=0)
    flat1, roots1, model1 = _annotated('F81')
    np.random.seed(21)
    sample_scenarios(roots1, 'c', model1, n_repetitions=n_rep)
    assert np.array_equal(_states_of(flat), _states_of(flat1))
    flat2, roots2, model2 = _annotated('F81')
    per_rep = sample_histories.last_stats['bytes_per_repetition']
    monkeypatch.setenv('PASTML_AMD_DEVICE_BYTES', str(2 * per_rep * 300))
    np.random.seed(21)
    chunked = sample_histories(roots2, 'c', model2, n_repetitions=n_rep, branch_jumps=True)
    assert sample_histories.last_stats['repetitions_per_call'] == 300
    for key in ('times', 'jumps', 'branch_jumps'):
        assert np.array_equal(chunked[key], whole[key]), key
    assert np.array_equal(_states_of(flat2), _states_of(flat))
    monkeypatch.delenv('PASTML_AMD_DEVICE_BYTES')
    flat3, roots3, model3 = _annotated('F81')
    exact = ml.expected_history(roots3, 'c', model3)
    s = history_summary(whole)
    assert exact['tree_length'] == pytest.approx(whole['tree_length'], rel=1e-14)
    assert ((s['times']['lower'] <= exact['times']) & (exact['times'] <= s['times']['upper'])).all()
    assert ((s['jumps']['lower'] <= exact['jumps']) & (exact['jumps'] <= s['jumps']['upper'])).all()
    se = whole['times'].std(axis=0, ddof=1) / math.sqrt(n_rep)
    assert (np.abs(s['times']['mean'] - exact['times']) <= BOUND * se).all()
