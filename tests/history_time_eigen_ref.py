"""
TEST INFRASTRUCTURE: the exact dwell times, Markov jumps and lineage counts per time interval of the eigen-decomposed models
(pml_history_through_time_eigen, include/pastml_hip.h) in Python's ``decimal`` at 60 digits, by two routes.

``by_subdivision`` shares no segment formula with the device.  Every branch is subdivided at the boundaries by unary nodes with
all-ones masks -- such a node changes no likelihood and no posterior --, matrix_exact_ref.EigenOperator is built on the subdivided
tree and its ``t`` list overwritten with the exact Decimal lengths w (dist + tau) tf sf (tau is 0 in the subdivided tree), and the
per-branch sums of expected_history_eigen_ref.history (whole branches: X_n = l_n Phi(t'_n) r_n), restated here branch by branch
because history() returns their total only, are added up per bin.  ``lineages`` is the marginal posterior q of the inserted nodes.

``by_scaling`` is the header's own forms on the original tree in Decimals: X_seg = ls Phi(w t') rs with ls = l exp(d s1 t'),
rs = r exp(d r t'), and the two-factor lineage posterior (q_p where t' = 0).

``consistent``.  The two routes are the same model only where (1) two pieces of a branch compose to the whole branch,
P(a) P(b) = A E_a (Ainv A) E_b Ainv = P(a + b), which needs Ainv A = 1, and (2) the posteriors are those of the chain itself:
the sweeps' top-down form P x followed by a product with pi is the chain's x^T P only where pi_a P_ab = pi_b P_ba.  The doubles
numpy left in A, Ainv and pi give both to 1e-16 and no further, and on them the two routes -- two models that differ by that much --
agree to 1e-16.  With ``consistent`` both routes replace Ainv by the inverse of the given A at 60 digits (Newton's
X <- X (2 - A X) from the given Ainv, three steps: 1e-16 -> 1e-64) and take the posteriors from the outside vectors
g_n = (g_p o v_p / m_n)^T P(t'_n), g_root = pi, which asks nothing of pi; then they are one model and must agree to what 60 digits
leave (tests/test_history_time_eigen_ref.py).  The segment forms themselves ask for neither: o_n = q_p / m_n is the joint law of a
branch's two ends for any chain, given the true q_p.  Without it both routes take the doubles and the sweeps' form as the device
does: that is the reference of the GPU tests (by_scaling).

The fractions of a segment are exact here ((hi - lo) / h on Decimals of the given doubles); the device's are those quotients
rounded to a double, half an ulp each.
"""
import decimal
from decimal import Decimal
from types import SimpleNamespace

import numpy as np

import matrix_exact_ref as exact
from expected_history_eigen_ref import _D
from f81_exact_ref import _CONTEXT, ZERO, ONE   # (60 digits)
from history_time_ref import segments

assert _CONTEXT.prec == 60
TWO = Decimal(2)


def _operator(spec, dist, sf, tau, tf, consistent):
    op = exact.EigenOperator(spec, dist, sf, tau, tf)
    if consistent:
        twice = np.array([[TWO if i == j else ZERO for j in range(op.k)] for i in range(op.k)], dtype=object)
        for _ in range(3):
            op.Ainv = op.Ainv.dot(twice - op.A.dot(op.Ainv))
    return op


def _pass(op, flat, masks, pi, consistent):
    """expected_history_eigen_ref._vectors on a given operator: (v [N], message [N], q [N], ln L).  consistent: the posteriors
    from the chain's own outside vectors x^T P, not from the sweeps' P x and pi."""
    parent, first_child, n_children = flat.parent, flat.first_child, flat.n_children
    N, k = np.asarray(masks).shape
    allowed = np.asarray(masks) != 0
    v, message = [None] * N, [None] * N
    for n in reversed(range(N)):
        row = np.array([ONE if a else ZERO for a in allowed[n]], dtype=object)
        fc = int(first_child[n])
        for c in range(fc, fc + int(n_children[n])):
            row = row * message[c]
        v[n] = row
        if parent[n] >= 0:
            message[n] = op.apply(n, row)
    loglik = sum((pi.dot(v[int(r)]).ln() for r in flat.roots), ZERO)
    down, q = [None] * N, [None] * N
    for n in range(N):   # parents first
        p = int(parent[n])
        if p < 0:
            down[n] = pi if consistent else np.array([ONE] * k, dtype=object)
        else:
            x = np.array([dp * vp / m if vp else ZERO for dp, vp, m in zip(down[p], v[p], message[n])], dtype=object)
            down[n] = (x.dot(op.A) * op.exponentials(n)).dot(op.Ainv) if consistent else op.apply(n, x)
        lh = v[n] * down[n] if consistent else v[n] * down[n] * pi
        q[n] = lh / sum(lh, ZERO)
    return v, message, q, loglik


def _Phi(op, y, Ey):
    """Phi_cd(y) [k, k]: (Ey[c] - Ey[d]) / (d_c - d_d), or y Ey[d] where d_c == d_d exactly."""
    gap = op.d[:, None] - op.d[None, :]
    equal = gap == 0
    Phi = (Ey[:, None] - Ey[None, :]) * np.where(equal, ZERO, ONE / np.where(equal, ONE, gap))
    Phi[equal] = np.broadcast_to(y * Ey[None, :], (op.k, op.k))[equal]
    return Phi


def _ends(op, n, v, message, q_p):
    """(l_n, r_n) of the branch above n."""
    nz = [i for i, x in enumerate(v[n]) if x != 0]
    r = op.Ainv[:, nz].dot(v[n][nz])
    o = np.array([qi / mi if qi else ZERO for qi, mi in zip(q_p, message[n])], dtype=object)
    return o.dot(op.A), r


def _transforms(op, W, sf, rows):
    """times [M][k], jumps [M]{i: [k]} from the W_m."""
    Q = (op.A * op.d[None, :]).dot(op.Ainv)
    times, jumps = [], []
    for Wm in W:
        T1 = op.Ainv.T.dot(Wm)
        times.append(list((T1 * op.A).sum(axis=1) / sf))
        per_row = {}
        for i in rows:
            row = Q[i] * op.A.dot(T1[i])
            row[i] = ZERO
            per_row[i] = list(row)
        jumps.append(per_row)
    return times, jumps


def _rows(k, jump_rows):
    return list(range(k)) if jump_rows is None else sorted(set(int(i) for i in jump_rows))


def by_subdivision(flat, masks, spec, node_time, boundaries, sf=1., tau=0., tf=1., jump_rows=None, consistent=False):
    """dict(loglik, times [M][k], jumps [M]{i: [k]}, lineages [M + 1][k], bin_length [M]) as Decimals."""
    with decimal.localcontext(_CONTEXT):
        sf_d, tau_d, tf_d = _D(sf), _D(tau), _D(tf)
        k = len(spec['pi'])
        T = [_D(x) for x in boundaries]
        M = len(T) - 1
        t = [_D(x) for x in node_time]
        N = flat.n_nodes
        masks = np.asarray(masks)
        # the subdivided forest: children lists over the old ids 0 .. N - 1 and the inserted ids from N on
        children = {n: [] for n in range(N)}
        dist, label, at_boundary = {}, {}, {}

        def bin_of(a):
            if a < T[0] or a >= T[M]:
                return None
            return max(m for m in range(M) if T[m] <= a)

        next_id = N
        for n in range(N):
            p = int(flat.parent[n])
            if p < 0:
                continue
            d = _D(flat.dist[n]) + tau_d
            h = t[n] - t[p]
            assert h >= 0
            if h == 0:
                children[p].append(n)
                dist[n] = d
                label[n] = None if (t[n] < T[0] or t[n] > T[M]) else (M - 1 if t[n] == T[M] else bin_of(t[n]))
                continue
            above, a = p, t[p]
            for m in [m for m in range(M + 1) if t[p] <= T[m] < t[n]]:
                u = next_id
                next_id += 1
                children[u] = []
                children[above].append(u)
                dist[u] = (T[m] - a) / h * d
                label[u] = bin_of(a) if T[m] > a else None
                at_boundary[u] = m
                above, a = u, T[m]
            children[above].append(n)
            dist[n] = (t[n] - a) / h * d
            label[n] = bin_of(a)
        # parents first, the children of a node next to each other
        order = [int(r) for r in flat.roots]
        for n in order:
            order.extend(children[n])
        new_of = {old: new for new, old in enumerate(order)}
        total = len(order)
        assert total == next_id
        sub = SimpleNamespace(parent=np.full(total, -1, dtype=np.int64), first_child=np.zeros(total, dtype=np.int64),
                              n_children=np.zeros(total, dtype=np.int64), dist=[ZERO] * total, roots=np.arange(len(flat.roots)))
        sub_masks = np.ones((total, k), dtype=np.int8)
        for new, old in enumerate(order):
            kids = children[old]
            sub.n_children[new] = len(kids)
            if kids:
                sub.first_child[new] = new_of[kids[0]]
                assert [new_of[c] for c in kids] == list(range(new_of[kids[0]], new_of[kids[0]] + len(kids)))
            for c in kids:
                sub.parent[new_of[c]] = new
            if old in dist:
                sub.dist[new] = dist[old]
            if old < N:
                sub_masks[new] = masks[old]
        op = _operator(spec, [0.0] * total, sf, 0.0, tf, consistent)
        op.t = [x * tf_d * sf_d for x in sub.dist]
        v, message, q, lnl = _pass(op, sub, sub_masks, exact._dec_array(spec['pi']), consistent)
        W = [np.full((k, k), ZERO, dtype=object) for _ in range(M)]
        lineages = [[ZERO] * k for _ in range(M + 1)]
        length = [ZERO] * M
        for new, old in enumerate(order):
            p = int(sub.parent[new])
            if p < 0:
                continue
            if old in at_boundary:
                m = at_boundary[old]
                lineages[m] = [x + y for x, y in zip(lineages[m], q[new])]
            m = label[old]
            if m is None:
                continue
            length[m] += sub.dist[new] * tf_d
            if op.t[new] == 0:
                continue
            l, r = _ends(op, new, v, message, q[p])
            W[m] = W[m] + (l[:, None] * _Phi(op, op.t[new], op.exponentials(new))) * r[None, :]
        times, jumps = _transforms(op, W, sf_d, _rows(k, jump_rows))
        return dict(loglik=lnl, times=times, jumps=jumps, lineages=lineages, bin_length=length)


def by_scaling(flat, masks, spec, node_time, boundaries, sf=1., tau=0., tf=1., jump_rows=None, consistent=False):
    """The same dict by the segment forms of include/pastml_hip.h on the original tree."""
    with decimal.localcontext(_CONTEXT):
        sf_d, tau_d, tf_d = _D(sf), _D(tau), _D(tf)
        k = len(spec['pi'])
        M = len(boundaries) - 1
        op = _operator(spec, flat.dist, sf, tau, tf, consistent)
        v, message, q, lnl = _pass(op, flat, masks, exact._dec_array(spec['pi']), consistent)
        W = [np.full((k, k), ZERO, dtype=object) for _ in range(M)]
        lineages = [[ZERO] * k for _ in range(M + 1)]
        length = [ZERO] * M
        segs, points = segments(flat.parent, node_time, boundaries)
        ends = {}

        def scaled(x, fraction, n):
            return x * np.array([(d * fraction * op.t[n]).exp() for d in op.d], dtype=object)

        def branch(n):
            if n not in ends:
                ends[n] = _ends(op, n, v, message, q[int(flat.parent[n])])
            return ends[n]

        def point(m, n, s, u):
            if op.t[n] == 0:
                term = q[int(flat.parent[n])]
            else:
                l, r = branch(n)
                term = op.Ainv.T.dot(scaled(l, s, n)) * op.A.dot(scaled(r, u, n))
            lineages[m] = [x + y for x, y in zip(lineages[m], term)]

        for m, n, s1, w, r_frac, starts in segs:
            length[m] += w * (_D(flat.dist[n]) + tau_d) * tf_d
            if starts:
                point(m, n, s1, w + r_frac)
            if op.t[n] == 0:
                continue
            l, r = branch(n)
            y = w * op.t[n]
            Ey = np.array([(d * y).exp() for d in op.d], dtype=object)
            W[m] = W[m] + (scaled(l, s1, n)[:, None] * _Phi(op, y, Ey)) * scaled(r, r_frac, n)[None, :]
        for n, s, rest in points:
            point(M, n, s, rest)
        times, jumps = _transforms(op, W, sf_d, _rows(k, jump_rows))
        return dict(loglik=lnl, times=times, jumps=jumps, lineages=lineages, bin_length=length)

