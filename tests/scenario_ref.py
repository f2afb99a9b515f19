"""
Plain numpy restatement of the scenario sampler's draws (pml_kernels_scenarios.h, pml_sample_scenarios): a test helper, not
a test module.

Every draw is one word of a Philox-4x32-10 call keyed by the seed and counter (global repetition >> 2, caller's node id, 0,
SCEN_TAG): repetition g takes word g & 3, u = x * 2^-32.  With w_n[b] = BU_n[b] * pi_b * mask_n[b] (BU = 1 at tips):

* a root: the wave scan of its posterior row, bisected at u * (the scan's last entry);
* F81 family (P_n[b][a] = (1 - e) pi_a + [a = b] e): cdf = wave scan of w_n, S = its last entry; for parent state a
  move = ((1 - e) * S) * pi_a, stay = e * w_n[a], W = move + stay, t = u * W; the child keeps a when t < stay, else it is
  bisect(cdf, (t - stay) * (S / move));
* the matrix models: row a = the running sum, left to right over b, of w_n[b] * max(P_n[b][a], 0); W = its last entry; the
  child is bisect(row a, u * W);
* W not positive: the node's posterior row, summed left to right, bisected at u * (that sum); the draw is counted.

Every product is rounded before it is added (the kernel forms no FMA there), so the restatement is exact; the draws within
``near`` * W of a boundary of their table are listed all the same, as for the counts sampler.
"""
import numpy as np

from sampler_ref import philox4x32_10, wave_scan, bisect, _pooled_chi2, ALPHA, seed_key   # noqa: F401 (re-exported)

SCEN_TAG = 0x7363656e   # word 3 of the counter (the simulator's and the counts sampler's are other words)


def scen_uniforms(seed, key, g):
    """u of global repetition g of node `key` (broadcast) = word g & 3 of Philox((g >> 2, key, 0, SCEN_TAG)) * 2^-32."""
    g = np.asarray(g, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    w = philox4x32_10((g >> np.uint64(2), key, 0, SCEN_TAG), *seed_key(seed))
    word = np.broadcast_to(g & np.uint64(3), w.shape[1:]).astype(np.int64)
    x = np.take_along_axis(w, word[None], axis=0)[0]
    return x.astype(np.float64) * 2.0 ** -32


def weights(flat, masks, bu, pi):
    """w_n[b] = BU_n[b] * pi_b * mask_n[b], BU = 1 at tips: [N, k]."""
    tip = np.asarray(flat.n_children) == 0
    pi = np.asarray(pi, dtype=np.float64)
    return np.where(np.asarray(masks) > 0, np.where(tip[:, None], 1.0, np.asarray(bu, dtype=np.float64)) * pi[None, :], 0.0)


def conditional_tables(w, pi, E=None, P=None):
    """
    The tables of nodes with weights w [m, k]: F81 family (E [m]) -> (cdf [m, k], S [m]); matrix models (P [m, k, k],
    P[i][b][a] = P_i(b -> a)) -> rows [m, k (parent state), k], the running sums left to right.
    """
    if E is not None:
        cdf, _ = wave_scan(w)
        return cdf, cdf[..., -1]
    terms = w[:, None, :] * np.maximum(np.transpose(np.asarray(P, dtype=np.float64), (0, 2, 1)), 0.0)
    return np.cumsum(terms, axis=-1)


def conditional_probabilities(flat, masks, bu, pi, E=None, P=None):
    """
    cond[n][a][b]: the probability that the tables give child state b of node n under parent state a (the share of the scaled
    uniform's range that bisects to b; NaN rows where the weights sum to zero).  Roots: NaN.
    """
    pi = np.asarray(pi, dtype=np.float64)
    w = weights(flat, masks, bu, pi)
    N, k = w.shape
    if E is not None:
        cdf, S = conditional_tables(w, pi, E=np.asarray(E, dtype=np.float64))
        steps = np.diff(np.concatenate([np.zeros((N, 1)), cdf], axis=1), axis=1)       # [N, b]
        e = np.asarray(E, dtype=np.float64)
        move = ((1.0 - e) * S)[:, None] * pi[None, :]                                  # [N, a]
        stay = e[:, None] * w
        with np.errstate(divide='ignore', invalid='ignore'):
            cond = move[:, :, None] * (steps / S[:, None])[:, None, :]
            cond[:, np.arange(k), np.arange(k)] += stay
            cond /= (move + stay)[:, :, None]
    else:
        rows = conditional_tables(w, pi, P=P)
        steps = np.diff(np.concatenate([np.zeros((N, k, 1)), rows], axis=2), axis=2)
        with np.errstate(divide='ignore', invalid='ignore'):
            cond = steps / rows[:, :, -1:]
    cond[np.asarray(flat.parent) < 0] = np.nan
    return cond


def _margin(table, rows, b, target, scale):
    """Distance of `target` to the boundaries of entry b of table row `rows`, over `scale` (the last entry has no upper one)."""
    k = table.shape[-1]
    flat = table.reshape(-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        up = np.where(b < k - 1, np.abs(flat[rows * k + b] - target), np.inf)
        low = np.where(b > 0, np.abs(target - flat[rows * k + np.maximum(b - 1, 0)]), np.inf)
        return np.minimum(up, low) / scale


def _fallback(post_rows, u):
    """Rows of posteriors [M, k] summed left to right, bisected at u * the sum."""
    cum = np.cumsum(np.asarray(post_rows, dtype=np.float64), axis=-1)
    return bisect(cum, np.arange(len(u)), u * cum[:, -1])


def _draw_nodes(nodes, parent_of, ps_rows, w, post, pi, seed, g, E, P, near):
    """States of `nodes` [m] given their parents' states ps_rows [m, n_rep] (ignored for roots).
    Returns (states [m, n_rep], fallback [m, n_rep] bool, near [m, n_rep] bool)."""
    u = scen_uniforms(seed, nodes[:, None], g[None, :])
    n_rep = u.shape[1]
    out = np.empty(u.shape, dtype=np.int64)
    fell = np.zeros(u.shape, dtype=bool)
    close = np.zeros(u.shape, dtype=bool)
    root = parent_of < 0
    if root.any():
        ur = u[root]
        cdf, _ = wave_scan(post[nodes[root]])
        rows = np.repeat(np.arange(len(cdf)), n_rep)
        total = cdf[:, -1][rows]
        target = ur.ravel() * total
        b = bisect(cdf, rows, target)
        out[root] = b.reshape(ur.shape)
        close[root] = (_margin(cdf, rows, b, target, total) <= near).reshape(ur.shape)
    ch = ~root
    if ch.any():
        uc, nc = u[ch], nodes[ch]
        m = len(nc)
        a = ps_rows[ch].astype(np.int64)
        node_row = np.repeat(np.arange(m), n_rep)
        af, uf = a.ravel(), uc.ravel()
        if E is not None:
            cdf, S = conditional_tables(w[nc], pi, E=E[nc])
            e = np.asarray(E, dtype=np.float64)[nc]
            rest = ((1.0 - e) * S)[node_row]
            Sf = S[node_row]
            move = rest * np.asarray(pi, dtype=np.float64)[af]
            stay = e[node_row] * w[nc][node_row, af]
            W = move + stay
            ok = W > 0.0
            t = uf * W
            with np.errstate(divide='ignore', invalid='ignore'):
                target = (t - stay) * (Sf / move)
            keep = t < stay
            tgt = np.where(ok & ~keep, target, 0.0)
            drawn = bisect(cdf, node_row, tgt)
            b = np.where(keep, af, drawn)
            with np.errstate(divide='ignore', invalid='ignore'):
                margin = np.abs(t - stay) / W
                margin = np.where(keep, margin, np.minimum(margin, _margin(cdf, node_row, drawn, tgt, Sf)))
        else:
            rows_tab = conditional_tables(w[nc], pi, P=np.asarray(P)[nc])
            k = rows_tab.shape[-1]
            table = rows_tab.reshape(-1, k)
            rows = node_row * k + af
            W = table[rows, k - 1]
            ok = W > 0.0
            tgt = np.where(ok, uf * W, 0.0)
            b = bisect(table, rows, tgt)
            with np.errstate(divide='ignore', invalid='ignore'):
                margin = _margin(table, rows, b, tgt, W)
        if not ok.all():
            bad = np.flatnonzero(~ok)
            b[bad] = _fallback(post[nc][node_row[bad]], uf[bad])
            margin[bad] = np.inf
        out[ch] = b.reshape(uc.shape)
        fell[ch] = (~ok).reshape(uc.shape)
        close[ch] = (margin <= near).reshape(uc.shape)
    return out, fell, close


def _blocks(nodes, n_rep, k, budget=1 << 21):
    step = max(1, budget // max(1, n_rep, k * k))
    for i in range(0, len(nodes), step):
        yield nodes[i:i + step]


def scenarios(flat, masks, bu, post, pi, seed, n_rep, rep_offset=0, E=None, P=None, parent_states=None, near=1e-12):
    """
    The states [N, n_rep] of pml_sample_scenarios for the forest `flat` (node ids = the caller's ids = the draws' keys).
    masks [N, k] 0/1 (the ones the pass ran with), bu [N, k] bottom-up vectors (tips: ignored, 1), post [N, k] posteriors,
    pi [k] as handed to the library, E [N] = exp(-mu t') of every branch (F81 / JC / EFT) or P [N, k, k] with
    P[n][b][a] = P_n(b -> a) (the other models).
    parent_states (optional [N, n_rep]): draw every node given these parents' states instead of the restated ones -- one
    flipped draw changes its whole subtree in that repetition, so a device result is compared one level at a time.
    Returns dict(states [N, n_rep] int64, n_fallback, near = [(node, repetition, drawn state)] of the draws whose scaled
    uniform lay within near * W of a boundary of their table).
    """
    N = flat.n_nodes
    k = np.asarray(masks).shape[1]
    pi = np.asarray(pi, dtype=np.float64)
    post = np.asarray(post, dtype=np.float64)
    w = weights(flat, masks, bu, pi)
    g = np.uint64(rep_offset) + np.arange(n_rep, dtype=np.uint64)
    parent = np.asarray(flat.parent, dtype=np.int64)
    out = np.empty((N, n_rep), dtype=np.int64)
    n_fallback = 0
    near_draws = []
    if parent_states is not None:
        levels = [np.arange(N)]
        src = np.asarray(parent_states)
    else:
        off = flat.td_offsets
        levels = [np.arange(off[d], off[d + 1]) for d in range(len(off) - 1)]
        src = out
    for level in levels:
        for nodes in _blocks(level, n_rep, k):
            s, fell, close = _draw_nodes(nodes, parent[nodes], src[np.maximum(parent[nodes], 0)], w, post, pi, seed, g, E, P, near)
            out[nodes] = s
            n_fallback += int(fell.sum())
            for i, r in np.argwhere(close):
                near_draws.append((int(nodes[i]), int(r), int(s[i, r])))
    return dict(states=out, n_fallback=n_fallback, near=near_draws)


def transition_counts_loop(flat, states, k):
    """scenario_transition_counts by a Python loop over the branches and repetitions."""
    n_rep = states.shape[1]
    out = np.zeros((n_rep, k, k), dtype=np.int64)
    for n in range(flat.n_nodes):
        p = flat.parent[n]
        if p < 0:
            continue
        for r in range(n_rep):
            out[r, states[p, r], states[n, r]] += 1
    return out
