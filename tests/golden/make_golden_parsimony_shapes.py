#!/usr/bin/env python3
"""
Generates tests/golden/parsimony_shapes.npz by running the REAL reference's pastml.parsimony.parsimonious_acr (imported
unmodified the way make_golden.py imports the reference) on every case of tests/parsimony_shape_cases.py within its reach
(FIXTURE_CASES: all but the stars of 65534 and 65535 tips, on which its downpass, quadratic in the arity, does not end):

    python3 -B tests/golden/make_golden_parsimony_shapes.py

Stored per forest: <forest>_parent, the parent array (the test rebuilds the forest from the case module and checks it).  Per case
<forest>_k<k>_: annotation, packed words [columns, N, W] (bit s of word s // 64 = state s; node ids in forest-wide level order;
the columns are parsimony_shape_cases.columns_of(k): column 2 needs two states); selected, the sets of ACCTRAN, DOWNPASS and DELTRAN
inside MP, packed words [columns, N, 3, W] (the three sets of a node side by side: they differ little, and the file is a third
smaller for it); steps [3, columns].  For column 3 of `shapes`, under shapes_c3_, what parsimony_wide.npz stores per prediction
method, for MP / DOWNPASS / ACCTRAN / DELTRAN in a row -- six results, RESULT_ORDER: method, character, and per state count (k) steps,
num_scenarios (a decimal string), unresolved nodes, states per node -- and a method on its own selects the same sets as inside MP
(asserted here).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402,F401  (stand-ins for ete3 / Bio / itolapi, the reference on sys.path)
from pastml.parsimony import parsimonious_acr as rpars, STEPS  # noqa: E402

import parsimony_shape_cases as cases  # noqa: E402
from pastml_amd.batch import masks_from_words  # noqa: E402
from pastml_amd.hip import pack_masks  # noqa: E402

CHARACTER = 'ch'
# (prediction method, reported method, feature) of the six results of column 3 of `shapes`
RESULT_ORDER = [('MP', m, CHARACTER + '_' + m) for m in cases.METHODS] + [(m, m, CHARACTER) for m in ('DOWNPASS', 'ACCTRAN', 'DELTRAN')]


def run(flat, roots, states, ann, method):
    """(results, {method: packed sets [N, W]}) of the reference on one annotation (bool [N, k])."""
    k = len(states)
    s2i = {s: i for i, s in enumerate(states)}
    for i, n in enumerate(flat.nodes):
        if ann[i].any():
            n.add_feature(CHARACTER, set(states[ann[i]]))
        else:
            n.del_feature(CHARACTER)
    results = rpars(roots, CHARACTER, method, states, flat.n_nodes, flat.n_tips)
    sets = {}
    for r in results:
        sel = np.zeros((flat.n_nodes, k), dtype=np.int8)
        for i, n in enumerate(flat.nodes):
            for s in getattr(n, r['character']):
                sel[i, s2i[s]] = 1
        sets[r['method']] = pack_masks(sel, k)
    return results, sets


def main():
    sys.setrecursionlimit(100000)
    out = {}
    c3 = dict(steps=[], num_scenarios=[], num_unresolved_nodes=[], num_states_per_node_avg=[])
    for name in cases.FIXTURE_FORESTS:
        flat = cases.forest(name)
        roots = [flat.nodes[r] for r in flat.roots] if flat.nodes is not None else flat.to_tree_nodes()
        out[name + '_parent'] = np.asarray(flat.parent, dtype=np.int32)
        for k in cases.states_of(name):
            b = cases.build(name, k)
            tag = cases.tag(name, k)
            states = np.array(['s{:03d}'.format(i) for i in range(k)])
            selected = np.zeros((3,) + b['given'].shape, dtype=np.uint64)
            steps = np.zeros((3, len(b['cols'])), dtype=np.int64)
            for c, col in enumerate(b['cols']):
                ann = masks_from_words(b['given'][c], k).astype(bool)
                results, sets = run(flat, roots, states, ann, 'MP')
                assert [r['method'] for r in results] == list(cases.METHODS)
                for j, r in enumerate(results):
                    selected[j, c] = sets[r['method']]
                    steps[j, c] = r[STEPS]
                if name == 'shapes' and col == 3:
                    for field in c3.values():
                        field.append([])
                    for method in ('MP', 'DOWNPASS', 'ACCTRAN', 'DELTRAN'):
                        if method != 'MP':
                            results, sets = run(flat, roots, states, ann, method)
                            assert np.array_equal(sets[method], selected[cases.METHODS.index(method), c]), (tag, method)
                        for r in results:
                            assert (method, r['method'], r['character']) == RESULT_ORDER[len(c3['steps'][-1])]
                            c3['steps'][-1].append(r[STEPS])
                            c3['num_scenarios'][-1].append(str(int(r['num_scenarios'])))
                            c3['num_unresolved_nodes'][-1].append(r['num_unresolved_nodes'])
                            c3['num_states_per_node_avg'][-1].append(r['num_states_per_node_avg'])
            out[tag + 'annotation'] = b['given']
            out[tag + 'selected'] = np.ascontiguousarray(np.moveaxis(selected, 0, 2))
            out[tag + 'steps'] = steps
        print(name, flat.n_nodes, 'nodes', flush=True)
    out['shapes_c3_prediction_method'], out['shapes_c3_method'], out['shapes_c3_character'] = (np.array(v) for v in zip(*RESULT_ORDER))
    out['shapes_c3_k'] = np.array(cases.states_of('shapes'))
    for field, rows in c3.items():
        out['shapes_c3_' + field] = np.array(rows)
    path = os.path.join(HERE, 'parsimony_shapes.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
