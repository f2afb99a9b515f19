"""
TEST INFRASTRUCTURE: the exact gradient of ln L of the F81 family (pml_loglik_gradient, include/pastml_hip.h) restated in
Python's ``decimal`` at 60 digits, in the manner of f81_exact_ref.py, whose helpers it uses: the inputs are the doubles the
device gets, converted exactly (or Decimals, for the finite-difference checks of this restatement itself), nothing is rounded to
a double and nothing is rescaled.

    mu = 1 / (1 - pi . pi),  t'_n = (d_n + tau) tf sf,  e_n = exp(-mu t'_n)
    v_n: bottom-up vector (a tip: its mask),  s_n = pi . v_n,  m_n[i] = (1 - e_n) s_n + e_n v_n[i],  q_p: posterior of n's parent
    for every non-root n that is not flat:
        A_n = sum_i q_p[i] / m_n[i],  B_n = sum_i q_p[i] v_n[i] / m_n[i]       (terms with q_p[i] == 0 are zero)
        h_n = -mu e_n (B_n - s_n A_n)
    T0 = sum h_n,  T1 = sum h_n t'_n,  E[m] = sum (1 - e_n) A_n v_n[m] + sum over the roots of v_r[m] / (pi . v_r)
    d/d sf = T1 / sf,  d/d tau at fixed tf = T0 tf sf,  d/d tf = T1 / tf,  d/d pi_m = E[m] + 2 mu pi_m T1

A branch is flat where e_n, rounded to a double, is 1.0 (t' = 0, or below 1e-16): the device cannot tell it from a branch of
length zero, leaves it out and counts it (n_flat); so does this file.  With no flat branch the sums are the exact gradient.

Next to each component stands its gross sum, the same sum with every term replaced by a bound of its size, against which an
error is measured:  sum mu e_n (|B_n| + |s_n A_n|) for T0 and the same with the factor t'_n for T1, scaled as the component is;
E[m] itself, whose terms are non-negative, plus 2 mu pi_m times the gross of T1.
(The gross sum of the tau component carries no factor t'_n: T0's own terms have none, and with it the bound would leave a branch
of 1e-12 out of what its own rounding error is measured against.)
"""
import decimal
from decimal import Decimal

import numpy as np

from f81_exact_ref import _CONTEXT, ZERO, ONE, _dot

TWO = Decimal(2)


def _D(x):
    return x if isinstance(x, Decimal) else Decimal(float(x))


def _vectors(flat, masks, pi, sf, tau, tf):
    """The marginal pass on Decimals: (mu, t' [N], e [N], v [N][k], message [N][k] (None for roots), q [N][k], ln L)."""
    parent, first_child, n_children = flat.parent, flat.first_child, flat.n_children
    N = len(parent)
    k = len(pi)
    allowed = [[bool(x) for x in row] for row in np.asarray(masks)]
    mu = ONE / (ONE - _dot(pi, pi))
    tt = [(_D(d) + tau) * tf * sf for d in flat.dist]
    e = [(-mu * t).exp() for t in tt]
    v, message = [None] * N, [None] * N
    for n in reversed(range(N)):
        row = [ONE if a else ZERO for a in allowed[n]]
        fc = int(first_child[n])
        for c in range(fc, fc + int(n_children[n])):
            row = [x * m if x else x for x, m in zip(row, message[c])]
        v[n] = row
        if parent[n] >= 0:
            base = (ONE - e[n]) * _dot(pi, row)
            message[n] = [base + e[n] * x if x else base for x in row]
    loglik = sum((_dot(pi, v[int(r)]).ln() for r in flat.roots), ZERO)
    down, q = [None] * N, [None] * N
    for n in range(N):   # parents first
        p = int(parent[n])
        if p < 0:
            down[n] = [ONE] * k
        else:
            x = [dp * vp / m if vp else ZERO for dp, vp, m in zip(down[p], v[p], message[n])]
            base = (ONE - e[n]) * _dot(pi, x)
            down[n] = [base + e[n] * xi for xi in x]
        lh = [a * b * c for a, b, c in zip(v[n], down[n], pi)]
        total = sum(lh, ZERO)
        q[n] = [x / total for x in lh]
    return mu, tt, e, v, message, q, loglik


def loglik(flat, masks, pi, sf=1., tau=0., tf=1.):
    """ln L as a Decimal; every argument a double (converted exactly) or a Decimal."""
    with decimal.localcontext(_CONTEXT):
        return _vectors(flat, masks, [_D(x) for x in pi], _D(sf), _D(tau), _D(tf))[6]


def gradient(flat, masks, pi, sf=1., tau=0., tf=1.):
    """
    dict(loglik, sf, tau_fixed_tf, tf, pi [k], n_flat, and gross_sf, gross_tau_fixed_tf, gross_tf, gross_pi [k]) as Decimals
    (n_flat: int), for doubles or Decimals pi [k], sf, tau, tf and 0/1 masks [N, k].
    """
    with decimal.localcontext(_CONTEXT):
        pi = [_D(x) for x in pi]
        sf, tau, tf = _D(sf), _D(tau), _D(tf)
        k = len(pi)
        mu, tt, e, v, message, q, lnl = _vectors(flat, masks, pi, sf, tau, tf)
        T0 = T1 = G0 = G1 = ZERO
        E = [ZERO] * k
        n_flat = 0
        for n in range(len(tt)):
            p = int(flat.parent[n])
            if p < 0:
                s = _dot(pi, v[n])
                E = [x + y / s for x, y in zip(E, v[n])]
                continue
            if float(e[n]) == 1.0:
                n_flat += 1
                continue
            f = [qi / mi if qi else ZERO for qi, mi in zip(q[p], message[n])]
            A = sum(f, ZERO)
            B = _dot(f, v[n])
            s = _dot(pi, v[n])
            h = -mu * e[n] * (B - s * A)
            g = mu * e[n] * (abs(B) + abs(s * A))
            T0 += h
            T1 += h * tt[n]
            G0 += g
            G1 += g * tt[n]
            c = (ONE - e[n]) * A
            E = [x + c * y for x, y in zip(E, v[n])]
        return dict(loglik=lnl, n_flat=n_flat,
                    sf=T1 / sf, tau_fixed_tf=T0 * tf * sf, tf=T1 / tf, pi=[x + TWO * mu * p * T1 for x, p in zip(E, pi)],
                    gross_sf=G1 / sf, gross_tau_fixed_tf=G0 * tf * sf, gross_tf=G1 / tf,
                    gross_pi=[x + TWO * mu * p * G1 for x, p in zip(E, pi)])


def tau_factor(tau, forest_length, num_nodes):
    """calc_tau_factor's formula (pastml/models/__init__.py:39-42) on Decimals; 1 at tau = 0, as there."""
    with decimal.localcontext(_CONTEXT):
        L, tau = _D(forest_length), _D(tau)
        return L / (L + tau * (int(num_nodes) - 1))


def chain_rule(grad, pi, tau, forest_length, num_nodes, free_sf=True, free_tau=False, free_frequencies=True):
    """
    The gradient with respect to the optimiser's vector [sf] [tau] [x_i = pi_i / pi_last, i < k - 1], for the parts that are
    free, from gradient()'s dict: (values, gross sums), lists of Decimals.
        d/d tau (total) = d/d tau at fixed tf + d/d tf * d tf/d tau,  d tf/d tau = -tf^2 (N - 1) / L
        d/d x_i = (g_i - pi . g) / (1 + sum x)
    The tau entry is NaN where grad['n_flat'] > 0.
    """
    with decimal.localcontext(_CONTEXT):
        pi = [_D(x) for x in pi]
        values, gross = [], []
        if free_sf:
            values.append(grad['sf'])
            gross.append(grad['gross_sf'])
        if free_tau:
            tf = tau_factor(tau, forest_length, num_nodes)
            slope = tf * tf * (int(num_nodes) - 1) / _D(forest_length)
            values.append(Decimal('NaN') if grad['n_flat'] else grad['tau_fixed_tf'] - grad['tf'] * slope)
            gross.append(grad['gross_tau_fixed_tf'] + grad['gross_tf'] * slope)
        if free_frequencies:
            S = ONE + sum((x / pi[-1] for x in pi[:-1]), ZERO)
            mean, gross_mean = _dot(pi, grad['pi']), _dot(pi, grad['gross_pi'])
            values += [(g - mean) / S for g in grad['pi'][:-1]]
            gross += [(g + gross_mean) / S for g in grad['gross_pi'][:-1]]
        return values, gross


def error_ratios(values, exact, gross):
    """|value - exact| / gross per component, floats, for doubles ``values`` against Decimals (NaN against NaN: 0)."""
    out = []
    with decimal.localcontext(_CONTEXT):
        for x, y, g in zip(np.atleast_1d(values), exact, gross):
            if y.is_nan() or np.isnan(x):
                out.append(0.0 if y.is_nan() and np.isnan(x) else np.inf)
            else:
                out.append(float(abs(Decimal(float(x)) - y) / g) if g > 0 else (0.0 if Decimal(float(x)) == y else np.inf))
    return np.array(out)
