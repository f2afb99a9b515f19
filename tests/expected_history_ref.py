"""
TEST INFRASTRUCTURE: the exact expected dwell times and Markov jumps of the F81 family (pml_expected_history,
include/pastml_hip.h) restated in Python's ``decimal`` at 60 digits, on the vectors of loglik_gradient_ref._vectors: the inputs
are the doubles the device gets, converted exactly, nothing is rounded to a double and nothing is rescaled.

    mu = 1 / (1 - pi . pi),  t'_n = (d_n + tau) tf sf,  L_n = (d_n + tau) tf,  x_n = mu t'_n,  e_n = exp(-x_n)
    v_n: bottom-up vector (a tip: its mask),  S_n = pi . v_n,  m_n[i] = (1 - e_n) S_n + e_n v_n[i],  q_p: posterior of n's parent
    o_n[i] = q_p[i] / m_n[i]  (0 where q_p[i] == 0),  O_n = sum_i o_n[i]
    g = (1 - e) / x,  c0 = 1 - 2 g + e,  c1 = g - e
    a_n[i] = pi_i O_n S_n c0 + o_n[i] S_n c1,   b_n[i] = pi_i O_n c1 + o_n[i] e_n
    times[s]        = sum_n L_n (a_n[s] + b_n[s] v_n[s])
    jumps[i][j]     = sum_n x_n pi_j (a_n[i] + b_n[i] v_n[j])   (i != j; 0 on the diagonal)
    branch_jumps[n] = x_n sum_i (a_n[i] (1 - pi_i) + b_n[i] (S_n - pi_i v_n[i]))   (a root: 0)

A branch with t' = 0 adds nothing.  At 60 digits the closed forms of c0 and c1 keep 30 digits on a branch of 1e-15.
"""
import decimal
from decimal import Decimal

import numpy as np

from f81_exact_ref import _CONTEXT, ZERO, ONE, _dot
from loglik_gradient_ref import _D, _vectors

TWO = Decimal(2)


def _vectors_stored(flat, masks, pi, sf, tau, tf, stored_e):
    """
    loglik_gradient_ref._vectors with the sweeps' e_n given (the doubles the device stored, converted exactly) instead of
    exp(-mu t'_n): what the marginal pass computes from its own rounded exponentials, without further rounding.  On a branch of
    1e-12 the stored e_n has 1 - e_n off by 1e-4 of itself, and the small entries of every vector above it follow.  The e
    returned is still the exact one: the explicit e_n, g, c0 and c1 of the sums are formed from x_n.
    """
    parent, first_child, n_children = flat.parent, flat.first_child, flat.n_children
    N, k = len(parent), len(pi)
    allowed = [[bool(x) for x in row] for row in np.asarray(masks)]
    mu = ONE / (ONE - _dot(pi, pi))
    tt = [(_D(d) + tau) * tf * sf for d in flat.dist]
    e = [_D(x) for x in stored_e]
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
    return mu, tt, [(-mu * t).exp() for t in tt], v, message, q, loglik


def history(flat, masks, pi, sf=1., tau=0., tf=1., jump_rows=None, stored_e=None):
    """
    dict(loglik, tree_length, times [k], jumps {i: [k]} for the rows i of ``jump_rows`` (None: every row), branch_jumps [N],
    posterior [N][k]) as Decimals, for doubles or Decimals pi [k], sf, tau, tf and 0/1 masks [N, k].
    stored_e [N] (doubles): the marginal pass on the exponentials the device stored (_vectors_stored) instead of exact ones.
    """
    with decimal.localcontext(_CONTEXT):
        pi = [_D(x) for x in pi]
        sf, tau, tf = _D(sf), _D(tau), _D(tf)
        k = len(pi)
        if stored_e is None:
            mu, tt, e, v, message, q, lnl = _vectors(flat, masks, pi, sf, tau, tf)
        else:
            mu, tt, e, v, message, q, lnl = _vectors_stored(flat, masks, pi, sf, tau, tf, stored_e)
        N = len(tt)
        rows = list(range(k)) if jump_rows is None else sorted(set(int(i) for i in jump_rows))
        times = [ZERO] * k
        jumps = {i: [ZERO] * k for i in rows}
        branch = [ZERO] * N
        length = ZERO
        for n in range(N):
            p = int(flat.parent[n])
            if p < 0:
                continue
            L = (_D(flat.dist[n]) + tau) * tf
            length += L
            x = mu * tt[n]
            if x == 0:
                continue
            g = (ONE - e[n]) / x
            c0 = ONE - TWO * g + e[n]
            c1 = g - e[n]
            S = _dot(pi, v[n])
            o = [qi / mi if qi else ZERO for qi, mi in zip(q[p], message[n])]
            O = sum(o, ZERO)
            a = [pi_i * O * S * c0 + o_i * S * c1 for pi_i, o_i in zip(pi, o)]
            b = [pi_i * O * c1 + o_i * e[n] for pi_i, o_i in zip(pi, o)]
            times = [t + L * (a_s + b_s * v_s) for t, a_s, b_s, v_s in zip(times, a, b, v[n])]
            for i in rows:
                row = jumps[i]
                jumps[i] = [r if j == i else r + x * pi[j] * (a[i] + b[i] * v[n][j]) for j, r in enumerate(row)]
            branch[n] = x * sum((a_i * (ONE - pi_i) + b_i * (S - pi_i * v_i) for a_i, b_i, pi_i, v_i in zip(a, b, pi, v[n])), ZERO)
        return dict(loglik=lnl, tree_length=length, times=times, jumps=jumps, branch_jumps=branch, posterior=q)


def identities(h, flat):
    """
    The two sides of I1, I2 (per state) and I3 of a full history() dict, as Decimals:
        I1: sum_s times[s] = tree_length;  I2: sum_j jumps[j][i] - sum_j jumps[i][j] = sum_n (q_n[i] - q_p(n)[i]);
        I3: sum_n branch_jumps[n] = sum_{i != j} jumps[i][j]
    as a list of (name, left, right, gross): gross the sum of the sizes of the terms of both sides.
    """
    with decimal.localcontext(_CONTEXT):
        k = len(h['times'])
        out = [('I1', sum(h['times'], ZERO), h['tree_length'], h['tree_length'])]
        q = h['posterior']
        for i in range(k):
            inflow = sum((h['jumps'][j][i] for j in range(k)), ZERO)
            outflow = sum(h['jumps'][i], ZERO)
            gain = loss = ZERO
            for n in range(len(q)):
                p = int(flat.parent[n])
                if p >= 0:
                    gain += q[n][i]
                    loss += q[p][i]
            out.append(('I2[{}]'.format(i), inflow - outflow, gain - loss, inflow + outflow + gain + loss))
        total = sum((sum(h['jumps'][i], ZERO) for i in range(k)), ZERO)
        out.append(('I3', sum(h['branch_jumps'], ZERO), total, total))
        return out


def relative_errors(values, exact):
    """|value - exact| / exact per entry, floats, for doubles ``values`` against non-negative Decimals; where the exact value
    is 0 the value has to be exactly 0 (inf otherwise)."""
    out = []
    with decimal.localcontext(_CONTEXT):
        for x, y in zip(np.asarray(values, dtype=np.float64).ravel(), exact):
            if not np.isfinite(x):
                out.append(np.inf)
            elif y == 0:
                out.append(0.0 if x == 0.0 else np.inf)
            else:
                out.append(float(abs(Decimal(float(x)) - y) / y))
    return np.array(out)
