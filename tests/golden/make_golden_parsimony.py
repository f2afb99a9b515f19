#!/usr/bin/env python3
"""
Generates tests/golden/parsimony_wide.npz by running the REAL reference's pastml.parsimony.parsimonious_acr (imported
unmodified the way make_golden.py imports the reference) on forests wider than those of parsimony.npz:

    python3 -B tests/golden/make_golden_parsimony.py

Cases, on FlatForest.random with zero_frac = 0.05; 10 % of the tips have no state, 10 % three states, the others one;
3 % of the internal nodes are annotated with one state (they tell "most common over all states, then intersect" from an
arg-max inside the node's own set, parsimony.py:92-122):

    a_   2 000 tips, k = 70, at most 6 children   (two words per set)
    b_   3 000 tips in 3 trees, k = 130, at most 9 children   (three words, counts beyond 8)
    c_  20 000 tips, k = 5, at most 3 children

Stored per case: the recipe of the forest and its parent array (the test rebuilds the forest from the recipe and checks
it), the states, the annotation as packed words [N, W] (bit s of word s // 64 = state s; node ids in forest-wide level
order), and for each of MP / DOWNPASS / ACCTRAN / DELTRAN the results in order: method, character, steps, num_scenarios
(a decimal string: it has thousands of digits), unresolved nodes, states per node.  The selected sets are stored once per
reconstruction, as packed words: a method on its own selects the same sets as inside MP (asserted here).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402,F401  (stand-ins for ete3 / Bio / itolapi, the reference on sys.path)
from pastml.parsimony import parsimonious_acr as rpars, STEPS  # noqa: E402

from pastml_amd.hip import pack_masks  # noqa: E402
from pastml_amd.tree import FlatForest  # noqa: E402

CASES = [('a_', dict(n_tips=2000, seed=21, max_arity=6, zero_frac=0.05, n_trees=1), 70, 31),
         ('b_', dict(n_tips=3000, seed=22, max_arity=9, zero_frac=0.05, n_trees=3), 130, 32),
         ('c_', dict(n_tips=20000, seed=23, max_arity=3, zero_frac=0.05, n_trees=1), 5, 33)]
CHARACTER = 'ch'


def annotation(flat, k, seed):
    """0/1 [N, k]: the annotated states of every node (all zero: none)."""
    rng = np.random.default_rng(seed)
    ann = np.zeros((flat.n_nodes, k), dtype=np.int8)
    for i in range(flat.n_nodes):
        u = rng.random()
        if flat.n_children[i] == 0:
            if u < 0.1:
                continue
            ann[i, rng.choice(k, size=min(3, k), replace=False) if u < 0.2 else int(rng.integers(k))] = 1
        elif u < 0.03:
            ann[i, int(rng.integers(k))] = 1
    return ann


def main():
    sys.setrecursionlimit(100000)
    out = {}
    for prefix, spec, k, seed in CASES:
        flat = FlatForest.random(**spec)
        roots = [flat.nodes[r] for r in flat.roots]
        states = np.array(['s{:03d}'.format(i) for i in range(k)])
        ann = annotation(flat, k, seed)
        out[prefix + 'spec'] = np.array([spec['n_tips'], spec['seed'], spec['max_arity'], spec['n_trees']])
        out[prefix + 'zero_frac'] = spec['zero_frac']
        out[prefix + 'parent'] = np.asarray(flat.parent, dtype=np.int32)
        out[prefix + 'states'] = states
        out[prefix + 'annotation'] = pack_masks(ann, k)
        s2i = {s: i for i, s in enumerate(states)}
        for method in ('MP', 'DOWNPASS', 'ACCTRAN', 'DELTRAN'):
            for i, n in enumerate(flat.nodes):
                if ann[i].any():
                    n.add_feature(CHARACTER, set(states[ann[i].astype(bool)]))
                else:
                    n.del_feature(CHARACTER)
            results = rpars(roots, CHARACTER, method, states, flat.n_nodes, flat.n_tips)
            out['{}{}_methods'.format(prefix, method)] = np.array([r['method'] for r in results])
            out['{}{}_characters'.format(prefix, method)] = np.array([r['character'] for r in results])
            out['{}{}_steps'.format(prefix, method)] = np.array([r[STEPS] for r in results], dtype=np.int64)
            out['{}{}_num_scenarios'.format(prefix, method)] = np.array([str(int(r['num_scenarios'])) for r in results])
            out['{}{}_num_unresolved_nodes'.format(prefix, method)] = np.array([r['num_unresolved_nodes'] for r in results])
            out['{}{}_num_states_per_node_avg'.format(prefix, method)] = np.array([r['num_states_per_node_avg'] for r in results])
            for r in results:
                sel = np.zeros((flat.n_nodes, k), dtype=np.int8)
                for i, n in enumerate(flat.nodes):
                    for s in getattr(n, r['character']):
                        sel[i, s2i[s]] = 1
                words = pack_masks(sel, k)
                key = '{}{}_selected'.format(prefix, r['method'])
                if key in out:
                    assert np.array_equal(out[key], words), (prefix, method, r['method'])
                out[key] = words
        print(prefix, flat.n_nodes, 'nodes', flush=True)
    path = os.path.join(HERE, 'parsimony_wide.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
