"""
TEST INFRASTRUCTURE: the small forests, masks and parameters the gradient tests share (host and GPU): the four shapes of
test_gpu_expected_counts.py plus one with zero-length branches, masks as there (one-hot tips, some missing, some with two
states).
"""
import numpy as np

from pastml_amd import synthetic
from pastml_amd.tree import FlatForest

SHAPES = ['balanced', 'ragged', 'polytomy', 'forest', 'zeros']


def forest(shape, seed=0):
    if shape == 'balanced':
        return synthetic.balanced_forest(5)
    if shape == 'ragged':
        return FlatForest.random(45, seed=3 + seed, max_arity=2, zero_frac=0.0, n_trees=1)
    if shape == 'polytomy':
        return FlatForest.random(50, seed=5 + seed, max_arity=5, zero_frac=0.0, n_trees=1)
    if shape == 'forest':
        return FlatForest.random(60, seed=7 + seed, max_arity=4, zero_frac=0.0, n_trees=3)
    if shape == 'zeros':
        return FlatForest.random(48, seed=9 + seed, max_arity=4, zero_frac=0.25, n_trees=2)
    raise ValueError(shape)


def host_forest(n_nodes_wanted, seed):
    """41 - 60 nodes with polytomies, two trees and zero-length branches (the host tests' forests)."""
    for n_tips in range(20, 60):
        flat = FlatForest.random(n_tips, seed=seed, max_arity=4, zero_frac=0.2, n_trees=2)
        if flat.n_nodes >= n_nodes_wanted:
            return flat
    raise ValueError(n_nodes_wanted)


def masks(flat, k, seed):
    """One-hot tips, some missing (all ones), some with two states; a tip on a zero-length branch is missing, so that the
    likelihood is positive at tau = 0 whatever its siblings show."""
    rng = np.random.default_rng(100 + seed)
    out = np.ones((flat.n_nodes, k), dtype=np.int8)
    tips = flat.tips
    out[tips] = 0
    out[tips, rng.integers(0, k, size=len(tips))] = 1
    out[tips[::9]] = 1
    for t in tips[4::11]:
        out[t, rng.integers(0, k)] = 1
    out[tips[flat.dist[tips] == 0]] = 1
    return out


def frequencies(kind, k, seed):
    if kind == 'JC':
        return np.full(k, 1.0 / k)
    return np.random.default_rng(1000 + 17 * k + seed).dirichlet(np.ones(k) * 2)


def rates(seed, tau):
    """(sf, tau, tau_factor)"""
    return 0.7 + 0.4 * seed, tau, 1.0 - 0.05 * (seed % 2)
