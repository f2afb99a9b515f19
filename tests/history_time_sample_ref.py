"""
Plain numpy restatement of the history sampler per time interval (pml_kernels_history_time_sample.h,
pml_sample_histories_through_time; the law is stated in include/pastml_hip.h): a test helper, not a test module.  Built on
history_sample_ref (event counts, words, branch scalars: the histories themselves are pml_sample_histories') and on the segments
of history_time_ref.segments, whose fractions are formed here as the device forms them, in doubles.  Conditioned on given
scenarios and stored exponentials.

    c_0 = 0, P_i = w_0 + .. + w_{i-1} left to right, c_i = P_i / Wsum (i = 1 .. M), c_{M+1} = 1 (set)
    segment (n, m): s1 = (lo - tp) / h, w = (hi - lo) / h; s2 = the s1 of (n, m + 1) (the point segment at T_M for m + 1 = M), or
        1 with the end included where there is none; h == 0: s1 = 0, w = 1, s2 = 1
    dwell of interval i in (n, m): L w if c_i <= s1 and s2 <= c_{i+1}, else L (min(c_{i+1}, s2) - max(c_i, s1)) where positive
    event i >= 1 at c_i counts in the segment with s1 <= c_i < s2 (or s1 <= c_i where the end is included)
    lineage of a segment with `starts`: the state s_i of the largest i with c_i <= s1
"""
import numpy as np

import history_sample_ref as hs
import history_time_ref as ht
from sampler_ref import wave_scan, bisect


def plan(parent, node_time, boundaries):
    """
    The segments of history_time_ref.segments, the points at T_M appended as segments of the pseudo-bin M, with the fractions
    in doubles as pml_plan_time_segments forms them and the upper ends of pml_time_segment_ends: dict of arrays bin, node, s1, w,
    s2, ends, starts, sorted by (bin, node).
    """
    T = np.asarray(boundaries, dtype=np.float64)
    t = np.asarray(node_time, dtype=np.float64)
    M = len(T) - 1
    segs, points = ht.segments(parent, node_time, boundaries)
    rows = []
    for m, n, s1d, wd, _, starts in segs:
        tp, tn = t[int(parent[n])], t[n]
        h = tn - tp
        if h == 0.0:
            s1, w = 0.0, 1.0
        else:
            lo, hi = max(T[m], tp), min(T[m + 1], tn)
            s1, w = (lo - tp) / h, (hi - lo) / h
        assert abs(s1 - float(s1d)) <= 1e-15 and abs(w - float(wd)) <= 1e-15 * max(1.0, float(wd) / 2.0 ** -40), (m, n)
        rows.append((m, n, s1, w, bool(starts)))
    for n, sd, _ in points:
        tp, tn = t[int(parent[n])], t[n]
        s1 = (T[M] - tp) / (tn - tp)
        assert abs(s1 - float(sd)) <= 1e-15
        rows.append((M, n, s1, 0.0, True))
    rows.sort(key=lambda row: (row[0], row[1]))
    first = {(m, n): s1 for m, n, s1, _, _ in rows}
    s2 = [first.get((m + 1, n), 1.0) for m, n, _, _, _ in rows]
    ends = [(m + 1, n) not in first for m, n, _, _, _ in rows]
    return dict(M=M, bin=np.array([r[0] for r in rows], dtype=np.int64), node=np.array([r[1] for r in rows], dtype=np.int64),
                s1=np.array([r[2] for r in rows], dtype=np.float64), w=np.array([r[3] for r in rows], dtype=np.float64),
                s2=np.array(s2, dtype=np.float64), ends=np.array(ends, dtype=bool),
                starts=np.array([r[4] for r in rows], dtype=bool))


def histories(flat, states, pi, E, sf, tau, tf, seed, node_time, boundaries, rep_offset=0, near=1e-12):
    """
    The outputs of pml_sample_histories_through_time on the scenarios `states` [N, n_rep]: dict(times [n_rep, M, k] float64,
    jumps [n_rep, M, k, k] uint32, lineages [n_rep, M + 1, k] uint32, summands [n_rep, M, k] -- the number of dwells added into
    each times entry --, scale [n_rep, M, k] -- the sum over the entry's cut pieces L (min - max) of (4 M_n + 16) 2^-52 L_n: such a
    piece is a difference of two positions, each a quotient of sums of up to M_n + 1 logs good to an ulp --, events [N, n_rep],
    near = the sorted (node, repetition) pairs history_sample_ref.histories lists, plus those with an event position within
    `near` of a segment end strictly inside (0, 1) -- a lineage point is a segment end --, n_skipped, whole = what
    history_sample_ref.histories returns for the same arguments).
    """
    whole = hs.histories(flat, states, pi, E, sf, tau, tf, seed, rep_offset, near)
    states = np.asarray(states).astype(np.int64)
    N, n_rep = states.shape
    pi = np.asarray(pi, dtype=np.float64)
    k = len(pi)
    E = np.asarray(E, dtype=np.float64)
    parent = np.asarray(flat.parent, dtype=np.int64)
    sp = plan(parent, node_time, boundaries)
    M_bins = sp['M']
    mu, x, L = hs.branch_scalars(flat, pi, sf, tau, tf)
    pcdf, _ = wave_scan(pi)
    ptotal = pcdf[-1]
    branch = np.flatnonzero(parent >= 0)
    branch = branch[~(x[branch] > hs.MAX_X)]
    # the histories, as history_sample_ref.histories draws them: pairs in (node, repetition) order, pair p has M + 1 intervals
    nn = np.repeat(branch, n_rep)
    rr = np.tile(np.arange(n_rep, dtype=np.int64), len(branch))
    gg = rr + int(rep_offset)
    a = states[parent[nn], rr]
    b = states[nn, rr]
    u0 = hs.words(seed, nn, gg, 0).astype(np.float64) * 2.0 ** -32
    M, _ = hs.event_counts(pi, E[nn], x[nn], a, b, u0, near)
    count = M + 1
    start = np.cumsum(count) - count
    pp = np.repeat(np.arange(len(nn)), count)
    ii = np.arange(int(count.sum()), dtype=np.int64) - start[pp]
    Mi = M[pp]
    drawn = Mi > 0
    X = hs.words(seed, nn[pp], gg[pp], 1 + ii).astype(np.float64)
    w = np.where(drawn, -np.log((X + 0.5) * 2.0 ** -32), 0.0)
    before = np.zeros(len(pp))                  # P_i
    run = np.zeros(len(nn))
    for i in range(int(M.max()) + 1 if len(M) else 0):   # left to right
        sel = np.flatnonzero((M >= i) & (M > 0))
        before[start[sel] + i] = run[sel]
        run[sel] = run[sel] + w[start[sel] + i]
    Wsum = run
    after = before + w                          # P_{i+1}
    with np.errstate(invalid='ignore', divide='ignore'):
        c_lo = np.where(ii == 0, 0.0, before / Wsum[pp])
        c_hi = np.where(ii == Mi, 1.0, after / Wsum[pp])
    s = np.where(ii == 0, a[pp], b[pp])
    inner = drawn & (ii > 0) & (ii < Mi)
    if inner.any():
        us = hs.words(seed, nn[pp][inner], gg[pp][inner], Mi[inner] + 1 + ii[inner]).astype(np.float64) * 2.0 ** -32
        s[inner] = bisect(pcdf[None], np.zeros(int(inner.sum()), dtype=np.int64), us * ptotal)
    prev = np.empty_like(s)
    prev[1:] = s[:-1]
    prev[:1] = s[:1]
    # every interval against every segment of its branch
    order = np.argsort(sp['node'], kind='stable')
    seg_count = np.bincount(sp['node'], minlength=N)
    seg_first = np.cumsum(seg_count) - seg_count
    per = seg_count[nn[pp]]
    iv = np.repeat(np.arange(len(pp)), per)
    off = np.cumsum(per) - per
    sg = order[seg_first[nn[pp][iv]] + (np.arange(int(per.sum()), dtype=np.int64) - off[iv])]
    s1, sw, s2, ends, starts, sbin = (sp[key][sg] for key in ('s1', 'w', 's2', 'ends', 'starts', 'bin'))
    point = sbin == M_bins
    lo_c, hi_c, st, pv, Lr, rep, ev, Mr = c_lo[iv], c_hi[iv], s[iv], prev[iv], L[nn[pp][iv]], rr[pp][iv], ii[iv], Mi[iv]
    contained = (lo_c <= s1) & (s2 <= hi_c) & ~point
    v = np.minimum(hi_c, s2) - np.maximum(lo_c, s1)
    cut = ~contained & ~point & (v > 0.0)
    dwell = np.where(contained, Lr * sw, Lr * v)
    add = contained | cut
    times = np.zeros((n_rep, M_bins, k))
    summands = np.zeros((n_rep, M_bins, k), dtype=np.int64)
    scale = np.zeros((n_rep, M_bins, k))
    np.add.at(times, (rep[add], sbin[add], st[add]), dwell[add])
    np.add.at(summands, (rep[add], sbin[add], st[add]), 1)
    np.add.at(scale, (rep[cut], sbin[cut], st[cut]), (4.0 * Mr[cut] + 16.0) * 2.0 ** -52 * Lr[cut])
    inside = (lo_c >= s1) & (ends | (lo_c < s2))
    jump = (ev > 0) & (st != pv) & ~point & inside
    flat_index = ((rep[jump] * M_bins + sbin[jump]) * k + pv[jump]) * k + st[jump]
    jumps = np.bincount(flat_index, minlength=n_rep * M_bins * k * k).astype(np.uint32).reshape(n_rep, M_bins, k, k)
    at = starts & (lo_c <= s1) & ((ev == Mr) | (hi_c > s1))
    flat_index = (rep[at] * (M_bins + 1) + sbin[at]) * k + st[at]
    lineages = np.bincount(flat_index, minlength=n_rep * (M_bins + 1) * k).astype(np.uint32).reshape(n_rep, M_bins + 1, k)
    close = np.zeros(len(pp), dtype=bool)
    for end in (s1, s2):
        hit = (ev > 0) & (end > 0.0) & (end < 1.0) & (np.abs(lo_c - end) <= near)
        close[iv[hit]] = True
    near_pairs = set(whole['near']) | set((int(nn[p]), int(rr[p])) for p in np.unique(pp[close]))
    events = np.zeros((N, n_rep), dtype=np.int64)
    events[nn, rr] = M
    return dict(times=times, jumps=jumps, lineages=lineages, summands=summands, scale=scale, events=events,
                near=sorted(near_pairs), n_skipped=whole['n_skipped'], whole=whole, plan=sp)


def bound(r):
    """The two parts of the bound on |times - r['times']|, added together (see histories)."""
    return (r['summands'] + 16) * 2.0 ** -52 * r['times'] + r['scale']
