"""
The decimal restatement of the exact gradient (tests/loglik_gradient_ref.py) held to central differences of a decimal ln L, its
chain rule to differences in the optimiser's variables, and the F81 models' own chain rule to it.  No GPU.

Central differences with step h = 1e-22 on 60-digit Decimals: the truncation error is of order h^2 = 1e-44 of the derivative,
the rounding error 1e-60 / 1e-22 = 1e-38 of ln L: the bound below is 1e-30 of the component's gross sum (or of |ln L| / h's
worth, whichever is larger), some eight digits above both and twenty below anything a dropped term would show.
"""
import decimal
from decimal import Decimal

import numpy as np
import pytest

import loglik_gradient_cases as cases
import loglik_gradient_ref as gref
from f81_exact_ref import _CONTEXT
from pastml_amd.annotation import ForestStats
from pastml_amd.models.F81Model import F81Model
from pastml_amd.models.JCModel import JCModel
from pastml_amd import synthetic

H = Decimal('1e-22')
BOUND = Decimal('1e-30')


def _case(k, tau, seed):
    flat = cases.host_forest(41 + 6 * seed, seed)
    assert 41 <= flat.n_nodes <= 60 and len(flat.roots) == 2
    assert flat.n_children.max() > 2, 'the case must have a polytomy'
    assert (flat.dist[flat.parent >= 0] == 0).any(), 'the case must have zero-length branches'
    masks = cases.masks(flat, k, seed)
    pi = cases.frequencies('F81', k, seed)
    sf, tau, tf = cases.rates(seed, tau)
    return flat, masks, pi, sf, tau, tf


def _central(f, x):
    return (f(x + H) - f(x - H)) / (2 * H)


@pytest.mark.parametrize('k', [2, 5, 17])
@pytest.mark.parametrize('tau', [0.0, 0.013])
def test_restatement_against_central_differences(k, tau):
    flat, masks, pi, sf, tau, tf = _case(k, tau, k % 3)
    g = gref.gradient(flat, masks, pi, sf, tau, tf)
    n_zero = int((flat.dist[flat.parent >= 0] == 0).sum())
    assert g['n_flat'] == (n_zero if tau == 0 else 0)
    with decimal.localcontext(_CONTEXT):
        D = [Decimal(float(x)) for x in pi]
        sf, tau, tf = Decimal(sf), Decimal(tau), Decimal(tf)
        checks = [('sf', g['sf'], g['gross_sf'], _central(lambda x: gref.loglik(flat, masks, D, x, tau, tf), sf)),
                  ('tf', g['tf'], g['gross_tf'], _central(lambda x: gref.loglik(flat, masks, D, sf, tau, x), tf))]
        if g['n_flat'] == 0:   # (the tau component is defined only there)
            checks.append(('tau', g['tau_fixed_tf'], g['gross_tau_fixed_tf'],
                           _central(lambda x: gref.loglik(flat, masks, D, sf, x, tf), tau)))
        for m in range(k):
            checks.append(('pi[{}]'.format(m), g['pi'][m], g['gross_pi'][m],
                           _central(lambda x: gref.loglik(flat, masks, D[:m] + [x] + D[m + 1:], sf, tau, tf), D[m])))
        for name, value, gross, fd in checks:
            assert gross > 0, name
            assert abs(value) <= gross * (1 + BOUND), name
            assert abs(value - fd) <= BOUND * gross, (name, value, fd)


def test_flat_branches_leave_sf_and_frequencies_exact():
    """At tau = 0 the zero-length branches are left out; the components other than tau are still the exact derivatives (checked
    above), and the count is the number of such branches -- also for a branch so short that exp(-mu t') rounds to 1.0."""
    flat, masks, pi, sf, tau, tf = _case(5, 0.0, 1)
    short = np.flatnonzero((flat.parent >= 0) & (flat.dist > 0))[:2]
    flat.dist[short] = 1e-18
    g = gref.gradient(flat, masks, pi, sf, tau, tf)
    assert g['n_flat'] == int((flat.dist[flat.parent >= 0] == 0).sum()) + 2


@pytest.mark.parametrize('k, free_tau', [(2, False), (5, True), (17, True)])
def test_chain_rule_against_differences_in_the_optimiser_variables(k, free_tau):
    flat, masks, pi, sf, tau, _ = _case(k, 0.013, k % 3)
    stats = ForestStats(flat)
    L, N = stats.forest_length, stats.num_nodes
    with decimal.localcontext(_CONTEXT):
        x0 = [Decimal(float(p)) / Decimal(float(pi[-1])) for p in pi[:-1]]
        sf, tau = Decimal(sf), Decimal(tau)

        def decode(x):
            S = 1 + sum(x, Decimal(0))
            return [v / S for v in x] + [1 / S]

        def lnl(sf_, tau_, x):
            return gref.loglik(flat, masks, decode(x), sf_, tau_, gref.tau_factor(tau_, L, N))

        D = decode(x0)
        g = gref.gradient(flat, masks, D, sf, tau, gref.tau_factor(tau, L, N))
        values, gross = gref.chain_rule(g, D, tau, L, N, free_sf=True, free_tau=free_tau, free_frequencies=True)
        fd = [_central(lambda v: lnl(v, tau, x0), sf)]
        if free_tau:
            fd.append(_central(lambda v: lnl(sf, v, x0), tau))
        for i in range(k - 1):
            fd.append(_central(lambda v: lnl(sf, tau, x0[:i] + [v] + x0[i + 1:]), x0[i]))
        assert len(values) == len(fd) == len(gross)
        for value, bound, d in zip(values, gross, fd):
            assert abs(value - d) <= BOUND * bound, (value, d)


def _stats_forest():
    flat = synthetic.balanced_forest(4)
    return flat, ForestStats(flat)


@pytest.mark.parametrize('k, free_tau, n_flat', [(2, False, 0), (5, True, 0), (5, True, 3), (17, True, 0)])
def test_model_method_against_the_restated_chain_rule(k, free_tau, n_flat):
    """F81Model.loglik_gradient_parameters on doubles against the Decimal chain rule on the same doubles: 1e-14 of the gross."""
    flat, stats = _stats_forest()
    rng = np.random.default_rng(k)
    pi = rng.dirichlet(np.ones(k) * 2)
    states = synthetic.state_names(k)
    model = F81Model(states=states, forest_stats=stats, sf=1.3, tau=0.02, optimise_tau=free_tau, frequencies=pi)
    d_rates, d_pi = rng.normal(size=3), rng.normal(size=k) * 10
    gross_rates, gross_pi = np.abs(d_rates) * 3, np.abs(d_pi) * 3
    with decimal.localcontext(_CONTEXT):
        g = dict(n_flat=n_flat, sf=Decimal(d_rates[0]), tau_fixed_tf=Decimal(d_rates[1]), tf=Decimal(d_rates[2]),
                 pi=[Decimal(x) for x in d_pi], gross_sf=Decimal(gross_rates[0]), gross_tau_fixed_tf=Decimal(gross_rates[1]),
                 gross_tf=Decimal(gross_rates[2]), gross_pi=[Decimal(x) for x in gross_pi])
    want, gross = gref.chain_rule(g, pi, model.tau, stats.forest_length, stats.num_nodes, free_sf=True, free_tau=free_tau,
                                  free_frequencies=True)
    got = model.loglik_gradient_parameters(d_rates, d_pi, n_flat)
    assert len(got) == len(model.get_optimised_parameters()) == len(want) == len(model.optimised_parameter_names())
    if free_tau:
        assert np.isnan(got[1]) == (n_flat > 0)
    ratios = gref.error_ratios(got, want, gross)
    assert ratios.max() < 1e-14, ratios.max()


def test_model_method_follows_what_is_free():
    flat, stats = _stats_forest()
    states = synthetic.state_names(4)
    d_rates, d_pi = np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0, 7.0])
    jc = JCModel(states=states, forest_stats=stats, sf=1.3)
    assert np.array_equal(jc.loglik_gradient_parameters(d_rates, d_pi, 0), [1.0])
    assert jc.optimised_parameter_names() == ['scaling_factor']
    jc.freeze()
    assert len(jc.loglik_gradient_parameters(d_rates, d_pi, 0)) == 0
    f81 = F81Model(states=states, forest_stats=stats, sf=1.3)
    f81.fix_extra_params()
    assert np.array_equal(f81.loglik_gradient_parameters(d_rates, d_pi, 0), [1.0])
    f81.unfix_extra_params()
    assert len(f81.loglik_gradient_parameters(d_rates, d_pi, 0)) == 4
    smoothed = F81Model(states=states, forest_stats=stats, sf=1.3, frequency_smoothing=True)
    with pytest.raises(NotImplementedError):
        smoothed.loglik_gradient_parameters(d_rates, d_pi, 0)
