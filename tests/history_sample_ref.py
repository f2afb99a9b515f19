"""
Plain numpy restatement of the history sampler's draws (pml_kernels_history_sample.h, pml_sample_histories; the law is stated in
include/pastml_hip.h): a test helper, not a test module.  It takes the states of the scenarios as given -- the device's in the
GPU tests, scenario_ref.scenarios in the host test -- and draws the history of every (branch, repetition) operation by
operation:

    mu = 1 / (1 - pi . pi) (the dot left to right),  d = d_n + tau,  x = mu (d (tf sf)),  L = d tf,  e = the stored E[n]
    draw d of (node, global repetition g) = word d & 3 of Philox((g, node, d >> 2, HSAMP_TAG)), u = X 2^-32
    M: x == 0 -> 0; q = 1.0 - e, u = draw 0; a != b: target = u q; a == b: Wa = q pi[a] + e, t = u Wa, t < e -> 0,
       else target = (t - e) / pi[a]; then term = e x, cum = term, m = 1; while cum <= target: m += 1, term = (term x) / m,
       stop if cum + term == cum or m == MAX_EVENTS, cum += term
    M >= 1: w_i = -log((X_{1+i} + 0.5) 2^-32), i = 0 .. M; Wsum left to right; dwell_i = (L w_i) / Wsum
            s_0 = a, s_M = b, s_i = bisect(wave_scan(pi), u_{M+1+i} * its last entry) for 0 < i < M
    M == 0: L to a
"""
import numpy as np

from sampler_ref import philox4x32_10, wave_scan, bisect, seed_key

HSAMP_TAG = 0x68697374
MAX_EVENTS = 4096
MAX_X = 512.0


def words(seed, node, g, d):
    """The 32-bit word of draw d of (node, global repetition g) (broadcast), as uint64."""
    node = np.asarray(node, dtype=np.uint64)
    g = np.asarray(g, dtype=np.uint64)
    d = np.asarray(d, dtype=np.uint64)
    w = philox4x32_10((g, node, d >> np.uint64(2), HSAMP_TAG), *seed_key(seed))
    word = np.broadcast_to(d & np.uint64(3), w.shape[1:]).astype(np.int64)
    return np.take_along_axis(w, word[None], axis=0)[0]


def branch_scalars(flat, pi, sf, tau, tf):
    """(mu, x [N], L [N]) as the device forms them."""
    dot = 0.0
    for p in np.asarray(pi, dtype=np.float64):
        dot += p * p
    mu = 1.0 / (1.0 - dot)
    d = np.asarray(flat.dist, dtype=np.float64) + float(tau)
    scale = float(tf) * float(sf)
    return mu, mu * (d * scale), d * float(tf)


def event_counts(pi, e, x, a, b, u, near):
    """M of pairs with parent state a, child state b, stored exponential e, x and uniform u (arrays of one length).
    Returns (M, close): close where the scaled uniform lies within near of its scale of the t < e decision or of a step of
    the walk."""
    pi = np.asarray(pi, dtype=np.float64)
    e, x, u = (np.asarray(v, dtype=np.float64) for v in (e, x, u))
    n = len(u)
    q = 1.0 - e
    same = a == b
    pa = pi[a]
    qa = q * pa
    Wa = qa + e
    t = u * Wa
    with np.errstate(divide='ignore', invalid='ignore'):
        target = np.where(same, (t - e) / pa, u * q)
        scale = np.where(same, Wa / pa, q)
    live = x != 0.0
    none = live & same & (t < e)
    walk = live & ~none
    close = live & same & (np.abs(t - e) <= near * Wa)
    M = np.zeros(n, dtype=np.int64)
    term = e * x
    cum = term.copy()
    lower = np.full(n, -np.inf)
    m = np.ones(n, dtype=np.int64)
    act = walk & (cum <= target)
    stopped = np.zeros(n, dtype=bool)    # left by the stop rule: no upper boundary
    while act.any():
        m[act] += 1
        tx = term * x
        with np.errstate(invalid='ignore'):
            new_term = tx / m
        term = np.where(act, new_term, term)
        nxt = cum + term
        stop = act & ((nxt == cum) | (m == MAX_EVENTS))
        stopped |= stop
        go = act & ~stop
        lower = np.where(go, cum, lower)
        cum = np.where(go, nxt, cum)
        act = go & (cum <= target)
    M[walk] = m[walk]
    with np.errstate(invalid='ignore'):
        margin = np.minimum(np.where(stopped, np.inf, np.abs(cum - target)), np.abs(target - lower)) / scale
    close |= walk & (margin <= near)
    return M, close


def histories(flat, states, pi, E, sf, tau, tf, seed, rep_offset=0, near=1e-12):
    """
    The outputs of pml_sample_histories on the scenarios `states` [N, n_rep] (node ids = the caller's ids = the draws' keys):
    dict(times [n_rep, k] float64, jumps [n_rep, k, k] uint32, branch_jumps [N, n_rep] uint16, summands [n_rep, k] -- the
    number of dwells added into each times entry --, events [N, n_rep] -- M of every branch and repetition --, near = the sorted
    (node, repetition) pairs one of whose scaled uniforms lies within `near` of its scale of a boundary: a step of the M walk, the
    t < e decision, a boundary of the pi table --, n_skipped = the branches with x > MAX_X, which are not drawn).
    """
    states = np.asarray(states).astype(np.int64)
    N, n_rep = states.shape
    pi = np.asarray(pi, dtype=np.float64)
    k = len(pi)
    E = np.asarray(E, dtype=np.float64)
    parent = np.asarray(flat.parent, dtype=np.int64)
    mu, x, L = branch_scalars(flat, pi, sf, tau, tf)
    pcdf, _ = wave_scan(pi)
    ptotal = pcdf[-1]
    branch = np.flatnonzero(parent >= 0)
    n_skipped = int((x[branch] > MAX_X).sum())
    branch = branch[~(x[branch] > MAX_X)]
    # pairs in (node, repetition) order
    nn = np.repeat(branch, n_rep)
    rr = np.tile(np.arange(n_rep, dtype=np.int64), len(branch))
    gg = rr + int(rep_offset)
    a = states[parent[nn], rr]
    b = states[nn, rr]
    u0 = words(seed, nn, gg, 0).astype(np.float64) * 2.0 ** -32
    M, close = event_counts(pi, E[nn], x[nn], a, b, u0, near)
    # the intervals: pair p has M + 1 of them
    count = M + 1
    start = np.cumsum(count) - count
    pp = np.repeat(np.arange(len(nn)), count)
    ii = np.arange(int(count.sum()), dtype=np.int64) - start[pp]
    Mi = M[pp]
    drawn = Mi > 0
    X = words(seed, nn[pp], gg[pp], 1 + ii).astype(np.float64)
    w = np.where(drawn, -np.log((X + 0.5) * 2.0 ** -32), 0.0)
    Wsum = np.zeros(len(nn))
    for i in range(int(M.max()) + 1 if len(M) else 0):   # left to right
        sel = np.flatnonzero((M >= i) & (M > 0))
        Wsum[sel] = Wsum[sel] + w[start[sel] + i]
    with np.errstate(invalid='ignore', divide='ignore'):
        dwell = np.where(drawn, (L[nn[pp]] * w) / Wsum[pp], L[nn[pp]])
    s = np.where(ii == 0, a[pp], b[pp])
    inner = drawn & (ii > 0) & (ii < Mi)
    if inner.any():
        us = words(seed, nn[pp][inner], gg[pp][inner], Mi[inner] + 1 + ii[inner]).astype(np.float64) * 2.0 ** -32
        at = us * ptotal
        zero = np.zeros(len(at), dtype=np.int64)
        si = bisect(pcdf[None], zero, at)
        s[inner] = si
        up = np.where(si < k - 1, np.abs(pcdf[si] - at), np.inf)
        low = np.where(si > 0, np.abs(at - pcdf[np.maximum(si - 1, 0)]), np.inf)
        edge = np.minimum(up, low) / ptotal <= near
        close[np.unique(pp[inner][edge])] = True
    times = np.zeros((n_rep, k))
    summands = np.zeros((n_rep, k), dtype=np.int64)
    np.add.at(times, (rr[pp], s), dwell)            # (in array order: per entry by node, then by interval)
    np.add.at(summands, (rr[pp], s), 1)
    prev = np.empty_like(s)
    prev[1:] = s[:-1]
    jump = (ii > 0) & (s != np.where(ii > 0, prev, s))
    flat_index = (rr[pp][jump] * k + prev[jump]) * k + s[jump]
    jumps = np.bincount(flat_index, minlength=n_rep * k * k).astype(np.uint32).reshape(n_rep, k, k)
    per_pair = np.bincount(pp[jump], minlength=len(nn))
    branch_jumps = np.zeros((N, n_rep), dtype=np.uint16)
    branch_jumps[nn, rr] = per_pair
    events = np.zeros((N, n_rep), dtype=np.int64)
    events[nn, rr] = M
    near_pairs = sorted((int(nn[p]), int(rr[p])) for p in np.flatnonzero(close))
    return dict(times=times, jumps=jumps, branch_jumps=branch_jumps, summands=summands, events=events, near=near_pairs,
                n_skipped=n_skipped)
