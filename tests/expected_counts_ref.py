"""
Plain numpy restatement of the exact expected transition counts (a test helper, not a test module).

What marginal_counts (pastml/ml.py:753-862) estimates by sampling, per node and term by term, from bottom-up vectors, the
root posteriors and P(t) -- the definition written into include/pastml_hip.h (pml_expected_counts) and
pastml_amd.ml.expected_counts.  The state frequencies q are PROPAGATED down the tree here (q_n = q_parent . M_n), as the
sampler's counts are; the device reads the posterior table instead, and the tests that compare the two show that this is
the same thing.  tests/test_expected_counts_ref.py holds this module to the reference's own 40 000-repetition estimates.
"""
import numpy as np


def to_initial(q, initial):
    """ml.py:806-812 / 840-846: q restricted to the states the altered node had, renormalised; those states evenly if
    nothing is left."""
    c = q * initial
    if np.count_nonzero(c):
        return c / c.sum()
    return initial / initial.sum()


def expected_counts(flat, masks, bu, posterior, pi, pij_of, altered=None, initial=None):
    """
    flat: FlatForest (level order: a parent's id is below its children's); masks [N, k] as the marginal pass ran with them;
    bu [N, k] bottom-up vectors (any per-node scale); posterior [N, k] (only the roots' rows are read); pij_of(n) = P_n
    [k, k] of the branch above n; altered: bool [N] or None; initial: [N, k] masks of the altered nodes before alteration.
    Returns dict(counts [k, k], q [N, k], uncorrected [k, k] (before the diagonal correction), branch_mass [k] = the sum over
    the branches of q_parent).
    """
    N, k = masks.shape
    pi = np.asarray(pi, dtype=np.float64)
    if altered is None:
        altered = np.zeros(N, dtype=bool)
    q = np.zeros((N, k))
    result = np.zeros((k, k))
    correction = np.zeros(k)
    branch_mass = np.zeros(k)
    for p in range(N):
        if flat.parent[p] < 0:
            q[p] = posterior[p] / posterior[p].sum()
        nc = flat.n_children[p]
        if nc == 0:
            continue
        ps = to_initial(q[p], initial[p]) if altered[p] else q[p]
        same = np.zeros(k)
        fc = flat.first_child[p]
        for n in range(fc, fc + nc):
            # M[a][b] ~ BU_n[b] pi_b mask_n[b] P_n[b][a]   (ml.py:819-824; P(0) of an eigen model clamped at zero)
            w = bu[n] * pi * masks[n]
            weights = w[None, :] * np.maximum(pij_of(n), 0.0).T
            den = weights.sum(axis=1)
            used = (q[p] > 0) & (den > 0)
            M = np.zeros((k, k))
            M[used] = weights[used] / den[used, None]
            q[n] = q[p].dot(M)
            branch_mass += np.where(used, q[p], 0.0)
            if not altered[p] and not altered[n]:
                result += q[p][:, None] * M
                same += q[p] * M.diagonal()
            else:
                ci = to_initial(q[n], initial[n]) if altered[n] else q[n]
                norm = ci / ci.sum()
                pos = ps > 0
                result[pos] += ps[pos, None] * norm[None, :]
                same[pos] += ps[pos] * norm[pos]
        correction += np.minimum(ps, same)
    counts = result.copy()
    counts[np.arange(k), np.arange(k)] -= correction
    return dict(counts=counts, q=q, uncorrected=result, branch_mass=branch_mass)


def from_oracle(orc, flat, masks, spec, sf=1., tau=0., tf=1., altered=None, initial=None):
    """The restatement on the oracle's own sweeps (oracle.pastml_oracle) for one character."""
    r = orc.full_marginal_pass(flat, masks, spec, sf=sf, tau=tau, tf=tf)
    out = expected_counts(flat, masks, r['bu'], r['posterior'], spec['pi'],
                          lambda n: orc.pij(spec, float(flat.dist[n]), sf, tau, tf), altered=altered, initial=initial)
    out['posterior'] = r['posterior']
    return out
