"""
Plain numpy restatement of the device samplers' draws (a test helper, not a test module).

The forward simulator (pml_kernels_simulate.h, pml_simulate_states) and the scenario sampler of marginal_counts
(pml_kernels_counts.h, pml_marginal_counts[_altered]) are deterministic: every draw is one Philox-4x32-10 call
(pml_philox.h) keyed by the seed, the caller's node id, the repetition or draw index and, for the counts sampler, the
parent state.  This module states that contract in vectorised numpy -- counters, word and bit mapping, the devices' scans
and bisection -- so that tests can compare the kernels draw for draw (tests/test_gpu_sampler_exact.py), and checks that
the contract is the right estimator (tests/test_sampler_ref.py).  The draws are defined by the global repetition / draw
index, not by how a kernel happens to fetch them.
"""
import numpy as np
from scipy import stats

M32 = 0xffffffff
SIM_TAG = 0x73696d75      # word 3 of the simulator's counter
COUNTS_TAG = 0x51ed270b   # word 3 of the counts sampler's counter
ROOT_STATE = 0xffffffff   # the counts sampler's "parent state" of a root's draws
# family-wise false-alarm probability of every chi-square family (Bonferroni over its tests)
ALPHA = 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# Philox-4x32-10 and the uniforms
# ---------------------------------------------------------------------------------------------------------------------

def philox4x32_10(ctr, k0, k1):
    """ctr: 4 arrays (or scalars, broadcast) of 32-bit counter words; k0, k1: the key words.  Returns uint64 [4, ...]."""
    c = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & np.uint64(M32) for x in ctr])
    c = [x.copy() for x in c]
    k0, k1 = int(k0) & M32, int(k1) & M32
    m32 = np.uint64(M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & m32
        hi1, lo1 = p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return np.stack(c)


def seed_key(seed):
    seed = int(seed)
    return seed & M32, (seed >> 32) & M32


def sim_uniforms(seed, key, g):
    """Simulator: u of global repetition g of node `key` (broadcast) = word g & 3 of Philox((g >> 2, key, 0, tag)) * 2^-32."""
    g = np.asarray(g, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    w = philox4x32_10((g >> np.uint64(2), key, 0, SIM_TAG), *seed_key(seed))
    word = np.broadcast_to(g & np.uint64(3), w.shape[1:]).astype(np.int64)
    x = np.take_along_axis(w, word[None], axis=0)[0]
    return x.astype(np.float64) * 2.0 ** -32


def counts_uniforms(seed, key, state, draw):
    """Counts sampler: u = ((w0 << 32 | w1) >> 11) * 2^-53 of Philox((draw, state, key, tag)) -- 53 bits, exact in a double."""
    w = philox4x32_10((draw, state, key, COUNTS_TAG), *seed_key(seed))
    bits = ((w[0] << np.uint64(32)) | w[1]) >> np.uint64(11)
    return bits.astype(np.float64) * 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------------
# the devices' cumulative sums and bisection
# ---------------------------------------------------------------------------------------------------------------------

def wave_scan(x):
    """
    The 64-lane wavefront scan of the kernels over the last axis: chunks of 64 lanes, zero-padded; in each chunk
    Hillis-Steele steps o = 1, 2, ..., 32 (every step reads the values from before it), then inc = scan + run with run the
    previous chunk's last lane.  Returns (inc [..., k], run = the last chunk's lane 63, which the counts sampler takes as
    its total).
    """
    x = np.asarray(x, dtype=np.float64)
    k = x.shape[-1]
    nch = (k + 63) // 64
    v = np.zeros(x.shape[:-1] + (nch * 64,))
    v[..., :k] = x
    v = v.reshape(x.shape[:-1] + (nch, 64))
    for o in (1, 2, 4, 8, 16, 32):
        v[..., o:] = v[..., o:] + v[..., :-o]   # (the right-hand side is formed before the assignment)
    run = np.zeros(x.shape[:-1])
    inc = np.empty_like(v)
    for c in range(nch):
        inc[..., c, :] = v[..., c, :] + run[..., None]
        run = inc[..., c, 63].copy()
    return inc.reshape(x.shape[:-1] + (nch * 64,))[..., :k], run


def seq_cumsum(x):
    """The simulator's matrix rows: run += max(P[a][b], 0) left to right (np.add.accumulate is sequential)."""
    return np.cumsum(np.maximum(np.asarray(x, dtype=np.float64), 0.0), axis=-1)


def bisect(table, rows, w):
    """The kernels' search: lo = 0, hi = k - 1; while lo < hi: mid = (lo + hi) >> 1, cdf[mid] > w ? hi = mid : lo = mid + 1.
    That is the first b with cdf[b] > w, else k - 1 (when the cdf is non-decreasing).  table [R, k], rows / w [M]."""
    table = np.asarray(table)
    k = table.shape[-1]
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    lo = np.zeros(w.shape, dtype=np.int64)
    hi = np.full(w.shape, k - 1, dtype=np.int64)
    flat = table.reshape(-1)
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi) >> 1
        gt = flat[rows * k + mid] > w
        hi = np.where(act & gt, mid, hi)
        lo = np.where(act & ~gt, mid + 1, lo)


# ---------------------------------------------------------------------------------------------------------------------
# forward simulation (pml_simulate_states)
# ---------------------------------------------------------------------------------------------------------------------

def _blocks(nodes, n_rep, budget=1 << 21):
    step = max(1, budget // max(1, n_rep))
    for i in range(0, len(nodes), step):
        yield nodes[i:i + step]


def _sim_nodes(nodes, parent_of, ps_rows, pcdf, ptotal, seed, g, E, P):
    """States of `nodes` [m] given their parents' states ps_rows [m, n_rep] (ignored for roots)."""
    u = sim_uniforms(seed, nodes[:, None], g[None, :])
    shape = u.shape
    out = np.empty(shape, dtype=np.int64)
    root = parent_of < 0
    if root.any():
        ur = u[root]
        out[root] = bisect(pcdf[None], np.zeros(ur.size, dtype=np.int64), (ur * ptotal).ravel()).reshape(ur.shape)
    ch = ~root
    if ch.any():
        uc, ps, nc = u[ch], ps_rows[ch].astype(np.int64), nodes[ch]
        if E is not None:
            e = E[nc][:, None]
            with np.errstate(divide='ignore'):
                scale = np.where(e < 1.0, ptotal / (1.0 - e), 0.0)
            w = (uc - e) * scale
            drawn = bisect(pcdf[None], np.zeros(w.size, dtype=np.int64), w.ravel()).reshape(w.shape)
            out[ch] = np.where(uc < e, ps, drawn)
        else:
            k = P.shape[-1]
            cdf = seq_cumsum(P[nc])                      # [m, k (parent state), k]
            rows = np.arange(len(nc))[:, None] * k + ps  # row a of node i
            total = cdf.reshape(-1, k)[rows, k - 1]
            out[ch] = bisect(cdf.reshape(-1, k), rows.ravel(), (uc * total).ravel()).reshape(uc.shape)
    return out


def simulate(flat, pi, seed, n_rep, rep_offset=0, E=None, P=None, parent_states=None):
    """
    States [N, n_rep] of pml_simulate_states for the forest `flat` (node ids = the caller's ids = the draws' keys).
    pi [k]: the column's frequencies as handed to the library; E [N]: exp(-mu t') of every branch (F81 / JC / EFT) or P
    [N, k, k] with P[n][a][b] = P_n(a -> b) (the other models).  Roots: bisect(pcdf, u * pcdf[-1]).  F81 family: the parent's
    state when u < e, else bisect(pcdf, (u - e) * (pcdf[-1] / (1 - e))).  Matrix models: bisect(row a, u * row a [-1]).
    parent_states (optional [N, n_rep]): draw every node given these parents' states instead of the restated ones.
    """
    pcdf, _ = wave_scan(np.asarray(pi, dtype=np.float64))
    ptotal = pcdf[-1]
    g = np.uint64(rep_offset) + np.arange(n_rep, dtype=np.uint64)
    N = flat.n_nodes
    out = np.empty((N, n_rep), dtype=np.int64)
    parent = np.asarray(flat.parent, dtype=np.int64)
    if parent_states is not None:
        src = np.asarray(parent_states)
        for nodes in _blocks(np.arange(N), n_rep):
            out[nodes] = _sim_nodes(nodes, parent[nodes], src[np.maximum(parent[nodes], 0)], pcdf, ptotal, seed, g, E, P)
        return out
    off = flat.td_offsets
    for d in range(len(off) - 1):
        for nodes in _blocks(np.arange(off[d], off[d + 1]), n_rep):
            out[nodes] = _sim_nodes(nodes, parent[nodes], out[np.maximum(parent[nodes], 0)], pcdf, ptotal, seed, g, E, P)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# scenario sampling (pml_marginal_counts / pml_marginal_counts_altered)
# ---------------------------------------------------------------------------------------------------------------------

def _draws(seed, keys, states, counts, cdf, W, rows_ok):
    """Draws of (key, state) pairs: counts[i] draws from cdf[i] scaled by W[i] (pairs with rows_ok False draw nothing).
    Returns (pair id, drawn state, margin = distance of the scaled uniform to its nearest cdf boundary / W) per draw."""
    counts = np.where(rows_ok, counts, 0).astype(np.int64)
    total = int(counts.sum())
    pair = np.repeat(np.arange(len(counts)), counts)
    start = np.cumsum(counts) - counts
    draw = np.arange(total, dtype=np.int64) - start[pair]
    u = counts_uniforms(seed, keys[pair], states[pair], draw) * W[pair]
    b = bisect(cdf, pair, u)
    k = cdf.shape[-1]
    flat = cdf.reshape(-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        up = np.where(b < k - 1, np.abs(flat[pair * k + b] - u), np.inf)
        low = np.where(b > 0, np.abs(u - flat[pair * k + np.maximum(b - 1, 0)]), np.inf)
        margin = np.minimum(up, low) / W[pair]
    return pair, b, margin


def counts(flat, masks, bu, post, pi, seed, n_rep, E=None, P=None, parent_counts=None, altered=None, near=1e-12):
    """
    The scenario sampler of pml_marginal_counts_altered (counts_roots_kernel / counts_level_kernel), node ids = the
    caller's.  masks [N, k] 0/1 (the current ones), bu [N, k] bottom-up vectors (tips: 1), post [N, k] (roots read),
    pi [k], E [N] (F81: P_n[b][a] = (1 - e) pi[a] + [a = b] e) or P [N, k, k] (P[n][b][a] = P_n(b -> a)).
    Roots: n_rep draws from the posterior, uniform keyed by state 0xffffffff.  A child n of parent p, for every a with
    pc[a] = counts[p][a] > 0: weights (bu pi mask)[b] * max(P_n[b][a], 0), wave-scanned; total W = lane 63; no draws if
    W = 0; draw i scales its uniform (keyed by (i, a, n)) by W and bisects.
    parent_counts (optional [N, k]): draw every child given these parents' counts (otherwise the restated ones).
    altered (optional [N] bool): pairs with an altered end add nothing to the sums; their parents ("dirty") keep their
    same-state draws in `same` instead of the diagonal correction.
    Returns dict(counts [N, k], sums [k, k] int64 (the device's integer sums), same [N, k], near = list of draws whose scaled
    uniform lay within near * W of a cdf boundary: (node, a, drawn b)).
    """
    N, k = masks.shape
    parent = np.asarray(flat.parent, dtype=np.int64)
    tip = np.asarray(flat.n_children) == 0
    pi = np.asarray(pi, dtype=np.float64)
    alt = np.zeros(N, dtype=bool) if altered is None else np.asarray(altered, dtype=bool)
    cnt = np.zeros((N, k), dtype=np.int64)
    sums = np.zeros((k, k), dtype=np.int64)
    same = np.zeros((N, k), dtype=np.int64)
    near_draws = []
    roots = np.flatnonzero(parent < 0)
    rcdf, rW = wave_scan(np.asarray(post, dtype=np.float64)[roots])
    for blk in _blocks(np.arange(len(roots)), n_rep):
        pair, b, margin = _draws(seed, roots[blk], np.full(len(blk), ROOT_STATE), np.full(len(blk), n_rep), rcdf[blk],
                                 rW[blk], np.ones(len(blk), dtype=bool))
        np.add.at(cnt, (roots[blk][pair], b), 1)
        for i in np.flatnonzero(margin <= near):
            near_draws.append((int(roots[blk][pair[i]]), -1, int(b[i])))
    base = np.where(masks > 0, np.where(tip[:, None], 1.0, np.asarray(bu, dtype=np.float64)) * pi[None, :], 0.0)
    if parent_counts is not None:
        levels = [np.flatnonzero(parent >= 0)]
    else:
        off = flat.td_offsets
        levels = [np.arange(off[d], off[d + 1]) for d in range(1, len(off) - 1)]
    for level in levels:
        for nodes in _blocks(level, n_rep * k, budget=1 << 22):
            src = cnt if parent_counts is None else np.asarray(parent_counts, dtype=np.int64)
            pc = src[parent[nodes]]                                  # [m, k]
            ni, a = np.nonzero(pc > 0)
            n = nodes[ni]
            if E is not None:
                e = np.asarray(E, dtype=np.float64)[n][:, None]
                pba = (1.0 - e) * pi[a][:, None] + np.where(np.arange(k)[None, :] == a[:, None], e, 0.0)
            else:
                pba = np.asarray(P)[n, :, a]                         # P_n[b][a] over b
            w = base[n] * np.maximum(pba, 0.0)
            cdf, W = wave_scan(w)
            pair, b, margin = _draws(seed, n, a, pc[ni, a], cdf, W, W > 0.0)
            np.add.at(cnt, (n[pair], b), 1)
            upd = ~(alt[parent[n]] | alt[n])
            keep = upd[pair]
            np.add.at(sums, (a[pair][keep], b[keep]), 1)
            diag = keep & (b == a[pair])
            np.add.at(same, (parent[n[pair][diag]], b[diag]), 1)
            for i in np.flatnonzero(margin <= near):
                near_draws.append((int(n[pair[i]]), int(a[pair[i]]), int(b[i])))
    # the diagonal correction of the clean parents; the dirty ones keep their same-state draws for the caller
    src = cnt if parent_counts is None else np.asarray(parent_counts, dtype=np.int64)
    internal = np.flatnonzero(~tip)
    dirty = alt.copy()
    ch = np.flatnonzero(parent >= 0)
    dirty[parent[ch][alt[ch]]] = True
    clean = internal[~dirty[internal]]
    corr = np.minimum(src[clean], same[clean]).sum(axis=0)
    sums[np.arange(k), np.arange(k)] -= corr
    same_out = np.zeros_like(same)
    same_out[internal[dirty[internal]]] = same[internal[dirty[internal]]]
    return dict(counts=cnt, sums=sums, same=same_out, near=near_draws)


def altered_assembly(flat, sums, state_counts, same, altered, initial_masks, n_rep):
    """
    marginal_counts on a forest with altered nodes, from the device's part (sums of the pairs without an altered end, per
    node state counts, same-state draws of the dirty parents): the pairs with an altered end get fractional counts.  An
    altered node's counts are first projected on its initial (unaltered) states and rescaled to n_rep -- or, if none of
    them is left, spread evenly over those states.  For a parent, each such child adds, for every parent state i with a
    positive (projected) count, that count times the child's normalised counts to row i, and its share of i to the
    parent's same-state tally; the parent then subtracts min(count, same-state tally) from the diagonal.
    Returns the k x k average per scenario.
    """
    alt = np.asarray(altered, dtype=bool)
    initial = np.asarray(initial_masks, dtype=np.float64)
    res = np.asarray(sums, dtype=np.float64).copy()
    k = res.shape[0]

    def project(c, node):
        v = c * initial[node]
        if np.any(v != 0):
            return n_rep * v / v.sum()
        return n_rep * initial[node] / initial[node].sum()

    for p in range(flat.n_nodes):
        kids = list(range(flat.first_child[p], flat.first_child[p] + flat.n_children[p]))
        if not kids or not (alt[p] or alt[kids].any()):
            continue
        pcs = np.asarray(state_counts[p], dtype=np.float64)
        if alt[p]:
            pcs = project(pcs, p)
        tally = np.asarray(same[p], dtype=np.float64).copy()
        for c in kids:
            if not (alt[p] or alt[c]):
                continue
            cc = np.asarray(state_counts[c], dtype=np.float64)
            if alt[c]:
                cc = project(cc, c)
            frac = cc / cc.sum()
            for i in range(k):
                if pcs[i] > 0:
                    add = frac * pcs[i]
                    res[i] += add
                    tally[i] += add[i]
        for i in range(k):
            res[i, i] -= min(pcs[i], tally[i])
    return res / n_rep


# ---------------------------------------------------------------------------------------------------------------------
# the statistical yardstick the restatement and the device are both held to
# ---------------------------------------------------------------------------------------------------------------------

def _pooled_chi2(observed, expected, min_expected=5.0):
    """Pearson chi-square p-value with cells of small expectation pooled into one (None: fewer than 2 cells)."""
    observed = np.asarray(observed, dtype=np.float64).ravel()
    expected = np.asarray(expected, dtype=np.float64).ravel()
    big = expected >= min_expected
    obs = list(observed[big])
    exp = list(expected[big])
    rest_o, rest_e = observed[~big].sum(), expected[~big].sum()
    if rest_e > 0:
        obs.append(rest_o)
        exp.append(rest_e)
    if len(exp) < 2:
        return None
    obs, exp = np.array(obs), np.array(exp)
    if exp.min() <= 0:
        return None
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    return float(stats.chi2.sf(chi2, len(exp) - 1))


def _check_transitions(flat, model, sim, k):
    """Roots against pi, every branch's (parent, child) table against n_a P[a][b] of the host model, Bonferroni."""
    pi = np.asarray(model.frequencies, dtype=np.float64)
    n_rep = sim.shape[1]
    tests = []
    for r in flat.roots:
        tests.append((np.bincount(sim[r], minlength=k), n_rep * pi / pi.sum()))
    for n in range(flat.n_nodes):
        p = flat.parent[n]
        if p < 0:
            continue
        P = np.maximum(model.get_Pij_t(float(flat.dist[n])), 0.0)
        P = P / P.sum(axis=1, keepdims=True)
        table = np.zeros((k, k))
        np.add.at(table, (sim[p].astype(np.int64), sim[n].astype(np.int64)), 1)
        n_a = table.sum(axis=1)
        tests.append((table, n_a[:, None] * P))
    pvals = [q for q in (_pooled_chi2(o, e) for o, e in tests) if q is not None]
    assert pvals, 'no testable cell'
    worst = min(pvals)
    assert worst > ALPHA / len(pvals), 'min p = {:.3g} over {} tests'.format(worst, len(pvals))
