#!/usr/bin/env python3
"""
Generates tests/golden/polytomies.npz by running the REAL reference's polytomy resolution (pastml/acr.py:234-278,
pastml/tree.py:344-492; imported unmodified the way make_golden.py imports the reference) here:

    python3 -B tests/golden/make_golden_polytomies.py

Part ``acr_``: acr(..., resolve_polytomies=True) on a seeded random two-tree forest with polytomies
(FlatForest.random, max arity 7, 5 % zero branches), dates annotated as the reference's pipeline does, five characters
in one call: F81 MPPA at fixed parameters (k = 5), JC MAP optimised (k = 3), EFT JOINT at a fixed scaling factor
(k = 4), DOWNPASS (k = 4) and COPY (k = 3).  The states are a seeded walk down the tree (see tip_table).  The
reference creates polytomy nodes and runs the unresolve loop (asserted below).  It keeps all of them: the new nodes
group children with equal predictions, mostly annotated tips, and the re-run gives them those children's states.  (Over
a hundred seeds, tip noise levels and missing fractions tried, none removed a node here.)  Removal is covered by part
``edit_``.
Stored: the input (forest recipe, annotation table, parameters); per node of the final forest in traverse order its name,
parent, dist, polytomy flag, selected states per result column and marginal probabilities; the scalars of every result;
the numbers of created and removed nodes per editing call.

Part ``edit_``: resolve_trees and then unresolve_trees alone on another random forest whose nodes carry prescribed
random state sets in three columns (some empty), new ones for the unresolve step; the topology after each call and the
return values.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

import make_golden as mg  # noqa: E402  (stand-ins for ete3 / Bio / itolapi, the reference on sys.path)
import pastml.acr as racr_module  # noqa: E402
from pastml.tree import annotate_dates, IS_POLYTOMY, resolve_trees as rresolve, unresolve_trees as runresolve  # noqa: E402

from pastml_amd.tree import FlatForest  # noqa: E402

# ---- part acr_
FOREST = dict(n_tips=1600, seed=4, max_arity=7, zero_frac=0.05, n_trees=2)
TIP_SEED = 11
MISSING = 0.05
# column, method, model, states, switching rate of the walk
CHARACTERS = [('f81', 'MPPA', 'F81', ['A', 'B', 'C', 'D', 'E'], 2.0),
              ('jc', 'MAP', 'JC', ['x', 'y', 'z'], 1.5),
              ('eft', 'JOINT', 'EFT', ['p', 'q', 'r', 's'], 2.0),
              ('mp', 'DOWNPASS', 'F81', ['g', 'h', 'i', 'j'], 1.5),
              ('cp', 'COPY', 'F81', ['u', 'v', 'w'], 1.0)]
F81_PARAMS = {'scaling_factor': 3.0, 'A': 0.3, 'B': 0.25, 'C': 0.2, 'D': 0.15, 'E': 0.1}
EFT_PARAMS = {'scaling_factor': 2.5}
# ---- part edit_
EDIT_FOREST = dict(n_tips=400, seed=7, max_arity=8, zero_frac=0.05, n_trees=2)
EDIT_SEED = 5
EDIT_STATES = {'a': ['0', '1', '2'], 'b': ['0', '1'], 'c': ['0', '1', '2', '3']}


def random_forest(spec):
    flat = FlatForest.random(spec['n_tips'], seed=spec['seed'], max_arity=spec['max_arity'],
                             zero_frac=spec['zero_frac'], n_trees=spec['n_trees'])
    return [flat.nodes[r] for r in flat.roots]


def tip_table(roots):
    """
    Node states: a walk down the tree (a state changes on a branch with probability 1 - exp(-rate * dist)).  The table
    has every node: the COPY column has a value on all of them (the reference copies the closest child's value onto a
    new polytomy node and fails where there is none, tree.py:411-412), the other columns on about 95 % of the tips.
    """
    rng = np.random.default_rng(TIP_SEED)
    nodes = [n for r in roots for n in r.traverse()]
    table = {}
    for column, method, _, states, rate in CHARACTERS:
        state = {}
        for r in roots:
            for n in r.traverse('preorder'):
                s = int(rng.integers(len(states))) if n.up is None else state[id(n.up)]
                if n.up is not None and rng.random() < 1 - np.exp(-rate * n.dist):
                    s = int(rng.integers(len(states)))
                state[id(n)] = s
        if method == 'COPY':
            table[column] = [states[state[id(n)]] for n in nodes]
        else:
            table[column] = [states[state[id(n)]] if n.is_leaf() and rng.random() >= MISSING else '' for n in nodes]
    return pd.DataFrame(table, index=pd.Index([n.name for n in nodes], name='id'))


def topology(roots):
    nodes = [n for r in roots for n in r.traverse()]
    return (np.array([n.name for n in nodes]), np.array([n.up.name if n.up is not None else '' for n in nodes]),
            np.array([n.dist for n in nodes], dtype=np.float64),
            np.array([bool(getattr(n, IS_POLYTOMY, False)) for n in nodes]))


def set_bits(nodes, column, states):
    s2i = {s: i for i, s in enumerate(states)}
    out = np.zeros((len(nodes), len(states)), dtype=np.int8)
    for i, n in enumerate(nodes):
        for s in getattr(n, column, set()):
            out[i, s2i[s]] = 1
    return out


def run_acr(seed):
    roots = random_forest(dict(FOREST, seed=seed))
    df = tip_table(roots)
    annotate_dates(roots)
    counts = dict(created=[], removed=[])

    def resolve(column2states, forest):
        counts['created'].append(rresolve(column2states, forest))
        return counts['created'][-1]

    def unresolve(column2states, forest):
        counts['removed'].append(runresolve(column2states, forest))
        return counts['removed'][-1]

    racr_module.resolve_trees, racr_module.unresolve_trees = resolve, unresolve
    np.random.seed(seed)
    try:
        results = racr_module.acr(roots, df.copy(), prediction_method=[c[1] for c in CHARACTERS],
                                  model=[c[2] for c in CHARACTERS],
                                  column2parameters={'f81': F81_PARAMS, 'eft': EFT_PARAMS}, threads=1,
                                  resolve_polytomies=True)
    finally:
        racr_module.resolve_trees, racr_module.unresolve_trees = rresolve, runresolve
    return roots, df, results, counts


def acr_part(out):
    roots, df, results, counts = run_acr(FOREST['seed'])
    assert counts['created'][0] > 0 and len(counts['removed']) >= 1
    names, parents, dist, polytomy = topology(roots)
    nodes = [n for r in roots for n in r.traverse()]
    out.update(acr_forest=np.array([FOREST[k] for k in ('n_tips', 'seed', 'max_arity', 'n_trees')]),
               acr_zero_frac=FOREST['zero_frac'], acr_table_names=np.array(df.index, dtype=str),
               acr_names=names, acr_parents=parents, acr_dist=dist, acr_polytomy=polytomy,
               acr_created=np.array(counts['created']), acr_removed=np.array(counts['removed']),
               acr_f81_params=np.array([F81_PARAMS['scaling_factor']] + [F81_PARAMS[s] for s in CHARACTERS[0][3]]),
               acr_eft_sf=EFT_PARAMS['scaling_factor'])
    for column, method, model, states, _ in CHARACTERS:
        out['acr_table_' + column] = np.array(df[column], dtype=str)
        out['acr_spec_' + column] = np.array([method, model] + states)
    out['acr_result_characters'] = np.array([r['character'] for r in results])
    for r in results:
        c = r['character']
        states = [str(s) for s in r['states']]
        out['acr_states_{}'.format(c)] = np.array(states)
        out['acr_selected_{}'.format(c)] = set_bits(nodes, c, states)
        for key, value in r.items():
            if key == 'marginal_probabilities':
                out['acr_marginal_{}'.format(c)] = value.loc[names, states].to_numpy(dtype=np.float64)
            elif key == 'model':
                out['acr_sf_{}'.format(c)] = float(value.sf)
                if hasattr(value, 'frequencies'):
                    out['acr_frequencies_{}'.format(c)] = np.asarray(value.frequencies, dtype=np.float64)
            elif isinstance(value, (int, float, np.floating, np.integer)) and not isinstance(value, bool):
                out['acr_scalar_{}__{}'.format(c, key)] = float(value)
    print('acr: {} nodes, created {}, removed {}'.format(len(names), counts['created'], counts['removed']))


def edit_part(out):
    roots = random_forest(EDIT_FOREST)
    annotate_dates(roots)
    rng = np.random.default_rng(EDIT_SEED)
    columns = sorted(EDIT_STATES)

    def prescribe(nodes, prefix, keep=0.0):
        for c in columns:
            states = EDIT_STATES[c]
            # mostly one state, drawn unevenly so that siblings often agree; sometimes two; a few nodes without any;
            # with probability ``keep`` a node keeps what it has
            p = np.linspace(2, 1, len(states))
            p /= p.sum()
            for n in nodes:
                u = rng.random()
                if rng.random() < keep:
                    continue
                if u < 0.03:
                    if c in n.features:
                        n.del_feature(c)
                    continue
                chosen = {int(rng.choice(len(states), p=p))}
                if u > 0.9:
                    chosen.add(int(rng.integers(len(states))))
                n.add_feature(c, {states[j] for j in chosen})
            out['{}sets_{}'.format(prefix, c)] = set_bits(nodes, c, states)

    nodes = [n for r in roots for n in r.traverse()]
    prescribe(nodes, 'edit_resolve_')
    column2states = {c: np.array(s) for c, s in EDIT_STATES.items()}
    created = rresolve(column2states, roots)
    names, parents, dist, polytomy = topology(roots)
    out.update(edit_forest=np.array([EDIT_FOREST[k] for k in ('n_tips', 'seed', 'max_arity', 'n_trees')]),
               edit_zero_frac=EDIT_FOREST['zero_frac'], edit_created=created, edit_resolved_names=names,
               edit_resolved_parents=parents, edit_resolved_dist=dist, edit_resolved_polytomy=polytomy)
    nodes = [n for r in roots for n in r.traverse()]
    prescribe(nodes, 'edit_unresolve_', keep=0.8)
    removed = runresolve(column2states, roots)
    names, parents, dist, polytomy = topology(roots)
    out.update(edit_removed=removed, edit_unresolved_names=names, edit_unresolved_parents=parents,
               edit_unresolved_dist=dist, edit_unresolved_polytomy=polytomy)
    print('edit: created {}, removed {}'.format(created, removed))
    assert created > 0 and 0 < removed < created


def main():
    out = {}
    edit_part(out)
    acr_part(out)
    path = os.path.join(HERE, 'polytomies.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
