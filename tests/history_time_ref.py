"""
TEST INFRASTRUCTURE: the exact dwell times, Markov jumps and lineage counts per time interval of the F81 family
(pml_history_through_time, include/pastml_hip.h) in Python's ``decimal`` at 60 digits, by two routes.

``by_subdivision`` shares no formula with the device.  Every branch is subdivided at the boundaries by unary nodes with all-ones
masks -- such a node changes no likelihood and no posterior --, the pieces get the lengths w (d + tau) as exact Decimals (tau is 0
in the subdivided tree, the tau factor stays), and the per-branch sums of expected_history_ref.history (whole branches: g, c0,
c1), restated here branch by branch because history() returns their totals only, are added up per bin.  ``lineages`` is the
marginal posterior q of the inserted nodes.

``by_coefficients`` is the header's own partial-branch forms (C0, C1a, C1b, Cee; A, B) on the original tree in Decimals; the
CPU test holds the two against each other to 1e-50, so the forms are proven before a GPU sees them.  It also runs on the
exponentials the device stored (expected_history_ref._vectors_stored).

The fractions of a segment are exact here ((hi - lo) / h on Decimals of the given doubles); the device's are those quotients
rounded to a double, half an ulp each.
"""
import decimal
from decimal import Decimal
from types import SimpleNamespace

import numpy as np

from expected_history_ref import _vectors_stored
from f81_exact_ref import _CONTEXT, ZERO, ONE, _dot
from loglik_gradient_ref import _D, _vectors

TWO = Decimal(2)


def segments(parent, node_time, boundaries):
    """
    Brute force over bins x nodes, on Decimals: (list of (bin, node, s1, w, r, starts), list of (node, s, 1 - s) alive at T_M).
    Sorted by (bin, node).
    """
    with decimal.localcontext(_CONTEXT):
        T = [_D(x) for x in boundaries]
        M = len(T) - 1
        t = [_D(x) for x in node_time]
        segs = []
        for m in range(M):
            for n in range(len(parent)):
                p = int(parent[n])
                if p < 0:
                    continue
                tp, tn = t[p], t[n]
                h = tn - tp
                if h == 0:
                    if T[m] <= tn < T[m + 1] or (m == M - 1 and tn == T[M]):
                        segs.append((m, n, ZERO, ONE, ZERO, False))
                    continue
                lo, hi = max(T[m], tp), min(T[m + 1], tn)
                if hi > lo:
                    segs.append((m, n, (lo - tp) / h, (hi - lo) / h, (tn - hi) / h, tp <= T[m]))
        points = []
        for n in range(len(parent)):
            p = int(parent[n])
            if p >= 0 and t[p] <= T[M] < t[n]:
                h = t[n] - t[p]
                points.append((n, (T[M] - t[p]) / h, (t[n] - T[M]) / h))
        return segs, points


def _whole_branch(pi, x, e, S, o, v):
    """a, b of expected_history_ref.history for one whole branch."""
    if x == 0:
        return None
    g = (ONE - e) / x
    c0 = ONE - TWO * g + e
    c1 = g - e
    O = sum(o, ZERO)
    a = [pi_i * O * S * c0 + o_i * S * c1 for pi_i, o_i in zip(pi, o)]
    b = [pi_i * O * c1 + o_i * e for pi_i, o_i in zip(pi, o)]
    return a, b


def _empty(M, k, rows):
    return ([[ZERO] * k for _ in range(M)], [{i: [ZERO] * k for i in rows} for _ in range(M)], [[ZERO] * k for _ in range(M + 1)],
            [ZERO] * M)


def _add(times, jumps, m, L, x, pi, a, b, v):
    times[m] = [t + L * (a_s + b_s * v_s) for t, a_s, b_s, v_s in zip(times[m], a, b, v)]
    for i, row in jumps[m].items():
        jumps[m][i] = [r if j == i else r + x * pi[j] * (a[i] + b[i] * v[j]) for j, r in enumerate(row)]


def by_subdivision(flat, masks, pi, node_time, boundaries, sf=1., tau=0., tf=1., jump_rows=None):
    """dict(loglik, times [M][k], jumps [M]{i: [k]}, lineages [M + 1][k], bin_length [M]) as Decimals."""
    with decimal.localcontext(_CONTEXT):
        pi = [_D(x) for x in pi]
        sf, tau, tf = _D(sf), _D(tau), _D(tf)
        k = len(pi)
        T = [_D(x) for x in boundaries]
        M = len(T) - 1
        t = [_D(x) for x in node_time]
        N = flat.n_nodes
        masks = np.asarray(masks)
        # the subdivided forest: children lists over the old ids 0 .. N - 1 and the inserted ids from N on
        children = {n: [] for n in range(N)}
        dist, label, at_boundary, is_old = {}, {}, {}, {}

        def bin_of(a):
            if a < T[0] or a >= T[M]:
                return None
            return max(m for m in range(M) if T[m] <= a)

        next_id = N
        for n in range(N):
            p = int(flat.parent[n])
            if p < 0:
                continue
            d = _D(flat.dist[n]) + tau
            h = t[n] - t[p]
            assert h >= 0
            if h == 0:
                children[p].append(n)
                dist[n] = d
                label[n] = None if (t[n] < T[0] or t[n] > T[M]) else (M - 1 if t[n] == T[M] else bin_of(t[n]))
                continue
            cuts = [m for m in range(M + 1) if t[p] <= T[m] < t[n]]
            above, a = p, t[p]
            for m in cuts:
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
                              n_children=np.zeros(total, dtype=np.int64), dist=[ZERO] * total,
                              roots=np.arange(len(flat.roots)))
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
        mu, tt, e, v, message, q, lnl = _vectors(sub, sub_masks, pi, sf, ZERO, tf)
        rows = list(range(k)) if jump_rows is None else sorted(set(int(i) for i in jump_rows))
        times, jumps, lineages, length = _empty(M, k, rows)
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
            L = sub.dist[new] * tf
            length[m] += L
            x = mu * tt[new]
            o = [qi / mi if qi else ZERO for qi, mi in zip(q[p], message[new])]
            ab = _whole_branch(pi, x, e[new], _dot(pi, v[new]), o, v[new])
            if ab is not None:
                _add(times, jumps, m, L, x, pi, ab[0], ab[1], v[new])
        return dict(loglik=lnl, times=times, jumps=jumps, lineages=lineages, bin_length=length)


def by_coefficients(flat, masks, pi, node_time, boundaries, sf=1., tau=0., tf=1., jump_rows=None, stored_e=None):
    """The same dict by the partial-branch forms of include/pastml_hip.h on the original tree; stored_e as history() takes it."""
    with decimal.localcontext(_CONTEXT):
        pi = [_D(x) for x in pi]
        sf, tau, tf = _D(sf), _D(tau), _D(tf)
        k = len(pi)
        M = len(boundaries) - 1
        if stored_e is None:
            mu, tt, e, v, message, q, lnl = _vectors(flat, masks, pi, sf, tau, tf)
        else:
            mu, tt, e, v, message, q, lnl = _vectors_stored(flat, masks, pi, sf, tau, tf, stored_e)
        rows = list(range(k)) if jump_rows is None else sorted(set(int(i) for i in jump_rows))
        times, jumps, lineages, length = _empty(M, k, rows)
        segs, points = segments(flat.parent, node_time, boundaries)

        def point(m, n, s, rest):
            p = int(flat.parent[n])
            x = mu * tt[n]
            A, B = ONE - (-s * x).exp(), ONE - (-rest * x).exp()
            S = _dot(pi, v[n])
            o = [qi / mi if qi else ZERO for qi, mi in zip(q[p], message[n])]
            O = sum(o, ZERO)
            lineages[m] = [l + (ONE - A) * (ONE - B) * o_j * v_j + (ONE - A) * B * o_j * S + A * (ONE - B) * pi_j * O * v_j +
                           A * B * pi_j * O * S for l, o_j, v_j, pi_j in zip(lineages[m], o, v[n], pi)]

        for m, n, s1, w, r, starts in segs:
            p = int(flat.parent[n])
            L = (_D(flat.dist[n]) + tau) * tf
            length[m] += w * L
            x = mu * tt[n]
            if starts:
                point(m, n, s1, w + r)
            y = w * x
            if y == 0:
                ey, c0, c1 = ONE, ZERO, ZERO
            else:
                ey = (-y).exp()
                g = (ONE - ey) / y
                c0, c1 = ONE - TWO * g + ey, g - ey
            A, B = ONE - (-s1 * x).exp(), ONE - (-r * x).exp()
            C0 = w * (c0 + (A + B) * c1 + A * B * ey)
            C1a = w * (ONE - A) * (c1 + B * ey)
            C1b = w * (ONE - B) * (c1 + A * ey)
            Cee = w * (ONE - A) * (ONE - B) * ey
            S = _dot(pi, v[n])
            o = [qi / mi if qi else ZERO for qi, mi in zip(q[p], message[n])]
            O = sum(o, ZERO)
            a = [pi_i * O * S * C0 + o_i * S * C1a for pi_i, o_i in zip(pi, o)]
            b = [pi_i * O * C1b + o_i * Cee for pi_i, o_i in zip(pi, o)]
            _add(times, jumps, m, L, x, pi, a, b, v[n])
        for n, s, rest in points:
            point(M, n, s, rest)
        return dict(loglik=lnl, times=times, jumps=jumps, lineages=lineages, bin_length=length)


def crossing(parent, node_time, boundaries):
    """int [M + 1]: the branches with time_p <= T_m < time_n."""
    parent = np.asarray(parent)
    t = np.asarray(node_time, dtype=np.float64)
    has = parent >= 0
    tp, tn = t[parent[has]], t[has]
    return np.array([int(((tp <= b) & (b < tn)).sum()) for b in boundaries])


def root_distance(flat, stagger=0.0):
    """float64 [N]: a node's time as the sum of the branch lengths above it (parents come first in a FlatForest); root number
    r begins at stagger * r."""
    t = np.zeros(flat.n_nodes)
    for r, n in enumerate(flat.roots):
        t[int(n)] = stagger * r
    for n in range(flat.n_nodes):
        p = int(flat.parent[n])
        if p >= 0:
            t[n] = t[p] + flat.dist[n]
    return t


def covering_boundaries(node_time, M, on_node=True):
    """M + 1 ascending boundaries from a little before the earliest node to a little after the latest, none lined up with a
    node -- but, with on_node, boundary M // 2 moved exactly onto a node time that lies between its neighbours."""
    t = np.asarray(node_time, dtype=np.float64)
    span = t.max() - t.min()
    b = t.min() - 0.013 * span + 1.031 * span * np.arange(M + 1) / M
    if on_node and M >= 2:
        m = M // 2
        inside = np.unique(t[(t > b[m - 1]) & (t < b[m + 1])])
        assert len(inside), 'no node time between the neighbours of boundary {}'.format(m)
        b[m] = inside[len(inside) // 2]
    assert (np.diff(b) > 0).all()
    return b
