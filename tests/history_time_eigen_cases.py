"""
TEST INFRASTRUCTURE: the inputs the tests of pml_history_through_time_eigen share (tests/test_history_time_eigen_ref.py on the
host, tests/test_gpu_history_time_eigen.py on the device).  Host arithmetic only.

nine_tips(): a ragged tree of 9 tips by hand -- a polytomy of four tips (n1), a node n1 whose branch has length 0 but an extent
of 0.07 (t' = 0 with h > 0 where tau = 0: its lineage term is the parent's posterior), a node n4 whose branch has length 0.05 and
no extent (h == 0: one whole segment) -- with its node times, and boundaries for M = 1, 3 and 7 that fall on a node's time, inside
a sliver of 1e-12 of a branch next to its parent and next to its child, and outside the tree on both sides.
"""
import numpy as np

from pastml_amd.models._eigen import JTT_FREQUENCIES, JTT_RATE_MATRIX, get_diagonalisation
from pastml_amd.tree import FlatForest, TreeNode

NEWICK = '((t1:0.11,t2:0.23,t3:0.05,t4:0.31)n1:0.0,((t5:0.17,t6:0.02)n3:0.13,t7:0.4)n2:0.21,(t8:0.09,t9:0.27)n4:0.05)root;'
EXTENT = {'n1': 0.07, 'n4': 0.0}   # time_n - time_p where it is not the branch length


def nine_tips():
    """(flat, node_time [N], {name: node id})"""
    flat = FlatForest.from_trees([TreeNode(NEWICK, format=1)])
    ids = {flat.nodes[i].name: i for i in range(flat.n_nodes)}
    extent = flat.dist.copy()
    for name, h in EXTENT.items():
        extent[ids[name]] = h
    t = np.zeros(flat.n_nodes)
    for n in range(flat.n_nodes):   # parents come first
        p = int(flat.parent[n])
        if p >= 0:
            t[n] = t[p] + extent[n]
    assert flat.n_tips == 9 and flat.n_children.max() == 4 and t[ids['n4']] == t[ids['root']]
    return flat, t, ids


def boundaries(flat, t, ids, M):
    """M + 1 ascending boundaries on the nine-tip tree.  M = 7: two bins before the root, a cut 1e-12 of n2's branch below the root
    (it also crosses n1's branch, whose t' is 0), n3's time exactly, a cut 1e-12 of t7's branch above t7, the last tip's time
    exactly -- and one bin beyond it; M = 3: the tree inside, the two slivers as bins of their own ends; M = 1: one bin that
    covers the tree."""
    def sliver(name, from_parent):
        n = ids[name]
        p = int(flat.parent[n])
        h = t[n] - t[p]
        return t[p] + 1e-12 * h if from_parent else t[n] - 1e-12 * h

    if M == 1:
        b = [t.min() - 0.1, t.max() + 0.1]
    elif M == 3:
        b = [sliver('n2', True), t[ids['n3']], sliver('t7', False), t.max() + 0.2]
    elif M == 7:
        b = [t.min() - 0.5, t.min() - 0.2, sliver('n2', True), t[ids['n3']], 0.45, sliver('t7', False), t.max(), t.max() + 0.5]
    else:
        raise ValueError(M)
    b = np.array(b, dtype=np.float64)
    assert (np.diff(b) > 0).all()
    return b


def masks(flat, k, seed):
    """One-hot tips, t3 missing (all ones), t6 with two states."""
    rng = np.random.default_rng(300 + seed)
    out = np.ones((flat.n_nodes, k), dtype=np.int8)
    tips = flat.tips
    out[tips] = 0
    out[tips, rng.integers(0, k, size=len(tips))] = 1
    out[tips[2]] = 1
    out[tips[5], rng.integers(0, k)] = 1
    return out


def jtt_spec():
    d, a, ainv = get_diagonalisation(JTT_FREQUENCIES, JTT_RATE_MATRIX)
    return dict(kind=2, pi=np.ascontiguousarray(JTT_FREQUENCIES, dtype=np.float64), d=np.ascontiguousarray(d, dtype=np.float64),
                A=np.ascontiguousarray(a, dtype=np.float64), Ainv=np.ascontiguousarray(ainv, dtype=np.float64))

