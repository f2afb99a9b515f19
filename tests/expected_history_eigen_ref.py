"""
TEST INFRASTRUCTURE: the exact expected dwell times and Markov jumps of the eigen-decomposed models (pml_expected_history_eigen,
include/pastml_hip.h) restated in Python's ``decimal`` at 60 digits with unbounded exponents, on the vectors of a marginal pass
built on matrix_exact_ref.EigenOperator: the inputs are the doubles the device gets (``pi``, ``d``, ``A``, ``Ainv``, ``sf``,
``tau``, ``tf``), converted exactly, nothing is rounded to a double and nothing is rescaled -- the rounding numpy left in A and
A^-1 is part of the model here, as it is for the device.

    Q = A diag(d) Ainv,  t'_n = (dist_n + tau) tf sf,  L_n = (dist_n + tau) tf
    v_n: bottom-up vector (a tip: its mask),  r_n = Ainv v_n,  E_n = exp(d t'_n),  m_n = A (E_n o r_n),  q_p: posterior of n's parent
    o_n[a] = q_p[a] / m_n[a]  (0 where q_p[a] == 0),  l_n = A^T o_n
    Phi_cd(t) = (E[c] - E[d]) / (d_c - d_d),  or  t exp(d_d t)  where d_c == d_d exactly
    X_n[c][d] = l_n[c] Phi_cd(t'_n) r_n[d],  W = sum_n X_n,  G = diag(d) - Ainv diag(Q_ii) A
    times[s]        = (1 / sf) sum_cd Ainv[c][s] W[c][d] A[s][d]
    jumps[i][j]     = Q_ij sum_cd Ainv[c][i] W[c][d] A[j][d]   (i != j; 0 on the diagonal)
    branch_jumps[n] = sum_cd G[c][d] X_n[c][d]                 (a root: 0)

A branch with t' = 0 adds nothing.  At 60 digits the difference quotient keeps 40 digits down to |(d_c - d_d) t| = 1e-20.
Nothing is clamped: an entry whose exact value is negative (A Ainv of the given doubles is not exactly 1) stays negative.

history_float64 restates the same sums in float64 numpy on given vectors, with the device's switch on |z|: the series of phi below
SWITCH, the difference quotient from it on.
"""
import decimal
from decimal import Decimal

import numpy as np

import matrix_exact_ref as exact
from f81_exact_ref import _CONTEXT, ZERO, ONE   # (60 digits)

assert _CONTEXT.prec == 60
SWITCH = 0.5    # PML_HEIG_SWITCH
TERMS = 15      # PML_HEIG_TERMS


def _D(x):
    return x if isinstance(x, Decimal) else Decimal(float(x))


def _vectors(flat, masks, spec, sf, tau, tf):
    """matrix_exact_ref.marginal_pass with the vectors kept as Decimals: (operator, v [N], message [N], q [N], ln L)."""
    parent, first_child, n_children = flat.parent, flat.first_child, flat.n_children
    N, k = np.asarray(masks).shape
    allowed = np.asarray(masks) != 0
    op = exact.EigenOperator(spec, flat.dist, sf, tau, tf)
    pi = exact._dec_array(spec['pi'])
    v, message, shared = [None] * N, [None] * N, {}
    for n in reversed(range(N)):
        row = np.array([ONE if a else ZERO for a in allowed[n]], dtype=object)
        fc = int(first_child[n])
        for c in range(fc, fc + int(n_children[n])):
            row = row * message[c]
        v[n] = row
        if parent[n] >= 0:
            key = (op.t[n], allowed[n].tobytes()) if n_children[n] == 0 else None
            if key is None or key not in shared:
                shared[key] = op.apply(n, row)
            message[n] = shared[key]
    loglik = sum((pi.dot(v[int(r)]).ln() for r in flat.roots), ZERO)
    down, q = [None] * N, [None] * N
    for n in range(N):   # parents first
        p = int(parent[n])
        if p < 0:
            down[n] = np.array([ONE] * k, dtype=object)
        else:
            key = (p, op.t[n], allowed[n].tobytes()) if n_children[n] == 0 else None
            if key is None or key not in shared:
                x = np.array([dp * vp / m if vp else ZERO for dp, vp, m in zip(down[p], v[p], message[n])], dtype=object)
                shared[key] = op.apply(n, x)
            down[n] = shared[key]
        lh = v[n] * down[n] * pi
        q[n] = lh / sum(lh, ZERO)
    return op, v, message, q, loglik


def history(flat, masks, spec, sf=1., tau=0., tf=1., jump_rows=None):
    """
    dict(loglik, tree_length, times [k], jumps {i: [k]} for the rows i of ``jump_rows`` (None: every row), branch_jumps [N],
    posterior [N][k], vectors [N][k]: the bottom-up vectors) as Decimals, for an eigen spec (matrix_exact_ref.KIND_EIGEN), doubles
    sf, tau, tf and 0/1 masks [N, k].
    """
    with decimal.localcontext(_CONTEXT):
        op, v, message, q, lnl = _vectors(flat, masks, spec, sf, tau, tf)
        A, Ainv, d = op.A, op.Ainv, op.d
        N, k = len(v), op.k
        tau_d, tf_d, sf_d = _D(tau), _D(tf), _D(sf)
        rows = list(range(k)) if jump_rows is None else sorted(set(int(i) for i in jump_rows))
        gap = d[:, None] - d[None, :]
        equal = gap == 0
        inv_gap = np.where(equal, ZERO, ONE / np.where(equal, ONE, gap))
        Q = (A * d[None, :]).dot(Ainv)
        G = np.diag(d) - (Ainv * Q.diagonal()[None, :]).dot(A)
        W = np.full((k, k), ZERO, dtype=object)
        branch = [ZERO] * N
        length = ZERO
        for n in range(N):
            p = int(flat.parent[n])
            if p < 0:
                continue
            length += (_D(flat.dist[n]) + tau_d) * tf_d
            t = op.t[n]
            if t == 0:
                continue
            nz = [i for i, x in enumerate(v[n]) if x != 0]
            r = Ainv[:, nz].dot(v[n][nz])
            E = op.exponentials(n)
            o = np.array([qi / mi if qi else ZERO for qi, mi in zip(q[p], message[n])], dtype=object)
            l = o.dot(A)
            Phi = (E[:, None] - E[None, :]) * inv_gap
            Phi[equal] = np.broadcast_to(t * E[None, :], (k, k))[equal]
            X = (l[:, None] * Phi) * r[None, :]
            W = W + X
            branch[n] = (G * X).sum()
        T1 = Ainv.T.dot(W)   # T1[s][d] = sum_c Ainv[c][s] W[c][d]
        times = list((T1 * A).sum(axis=1) / sf_d)
        jumps = {}
        for i in rows:
            row = Q[i] * A.dot(T1[i])
            row[i] = ZERO
            jumps[i] = list(row)
        return dict(loglik=lnl, tree_length=length, times=times, jumps=jumps, branch_jumps=branch,
                    posterior=[list(x) for x in q], vectors=[list(x) for x in v])


def scaled_errors(values, exact_values):
    """|value - exact| / (the largest |exact| of the array) per entry, floats: the sums have mixed signs, so an entry is held to
    the size of the array's largest one.  inf for a value that is not finite."""
    with decimal.localcontext(_CONTEXT):
        exact_values = list(exact_values)
        top = max(abs(y) for y in exact_values)
        out = []
        for x, y in zip(np.asarray(values, dtype=np.float64).ravel(), exact_values):
            if not np.isfinite(x):
                out.append(np.inf)
            elif top == 0:
                out.append(0.0 if x == 0.0 else np.inf)
            else:
                out.append(float(abs(Decimal(float(x)) - y) / top))
        return np.array(out)


def jumps_top(h):
    """The largest |entry| of the jump rows a history() holds."""
    with decimal.localcontext(_CONTEXT):
        return max(abs(x) for row in h['jumps'].values() for x in row)


def float_vectors(h):
    """(v [N, k], q [N, k]) of a history() as doubles, each bottom-up vector divided by its largest entry first (any scaling
    cancels; the exact vectors of a deep tree are below the doubles' range)."""
    with decimal.localcontext(_CONTEXT):
        v = np.array([[float(x / max(row)) for x in row] for row in h['vectors']])
        q = np.array([[float(x) for x in row] for row in h['posterior']])
    return v, q


def phi_series(z):
    """expm1(z) / z for 0 <= z < SWITCH: 1 + z / 2! + ... + z^15 / 16!, by Horner's rule as the device forms it."""
    inv = [1.0]
    f = 1.0
    for m in range(1, TERMS + 1):
        f *= m + 1
        inv.append(1.0 / f)
    s = np.full_like(z, inv[TERMS])
    for m in range(TERMS - 1, 0, -1):
        s = s * z + inv[m]
    return s * z + 1.0


def history_float64(flat, spec, sf, tau, tf, v, q, branch_jumps=True):
    """The sums of history() in float64 numpy on the vectors v [N, k] and posteriors q [N, k] given: dict(times [k], jumps
    [k, k], branch_jumps [N]).  Phi by the device's rule: below SWITCH t E[the smaller eigenvalue's] phi(|z|), else the quotient."""
    A, Ainv, d = (np.asarray(spec[key], dtype=np.float64) for key in ('A', 'Ainv', 'd'))
    k, N = len(d), len(flat.parent)
    Q = (A * d[None, :]).dot(Ainv)
    G = np.diag(d) - (Ainv * Q.diagonal()[None, :]).dot(A)
    gap = d[:, None] - d[None, :]
    W = np.zeros((k, k))
    branch = np.zeros(N)
    for n in range(N):
        p = int(flat.parent[n])
        t = (flat.dist[n] + tau) * (tf * sf)
        if p < 0 or t == 0:
            continue
        r = Ainv.dot(v[n])
        E = np.exp(d * t)
        m = A.dot(E * r)
        with np.errstate(divide='ignore', invalid='ignore'):
            o = np.where((q[p] > 0) & (m > 0), q[p] / m, 0.0)
            l = o.dot(A)
            z = gap * t
            small = t * np.where(z >= 0, E[None, :], E[:, None]) * phi_series(np.minimum(np.abs(z), SWITCH))
            Phi = np.where(np.abs(z) < SWITCH, small, (E[:, None] - E[None, :]) / gap)
        X = l[:, None] * Phi * r[None, :]
        W += X
        if branch_jumps:
            branch[n] = max((G * X).sum(), 0.0)
    T1 = Ainv.T.dot(W)
    times = np.maximum((T1 * A).sum(axis=1) / sf, 0.0)
    jumps = np.maximum(Q * T1.dot(A.T), 0.0)
    np.fill_diagonal(jumps, 0.0)
    return dict(times=times, jumps=jumps, branch_jumps=branch)


def f81_as_eigen(pi):
    """An F81 model handed over as an eigen model, through the symmetrised matrix and numpy.linalg.eigh: every non-zero eigenvalue
    equal (-mu), A = diag(1 / sqrt(pi)) U, Ainv = U^T diag(sqrt(pi))."""
    pi = np.asarray(pi, dtype=np.float64)
    mu = 1.0 / (1.0 - pi.dot(pi))
    root = np.sqrt(pi)
    sym = mu * (np.outer(root, root) - np.eye(len(pi)))
    d, u = np.linalg.eigh(sym)
    return dict(kind=exact.KIND_EIGEN, pi=pi, d=np.ascontiguousarray(d), A=np.ascontiguousarray(u / root[:, None]),
                Ainv=np.ascontiguousarray(u.T * root[None, :]))
