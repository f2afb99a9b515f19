#!/usr/bin/env python3
"""
Generates tests/golden/simulate_albania.npz by running the REAL reference's forward simulator
(pastml/utilities/state_simulator.py, imported unmodified the way make_golden.py imports the reference) on the 152-taxa
Albania tree, 20 000 repetitions, fixed numpy seed, under two models:

    F81  with the Country parameters of data/albania_pastml/params.character_Country.method_MPPA.model_F81.tab
    JTT  with the scaling factor of that file

    python3 -B tests/golden/make_golden_simulate.py

Only data is stored: node names (level order), per-node state histograms [N, k] and the summed (parent, child) transition
matrix [k, k] of each model.  tests/test_gpu_simulate.py compares the device's simulation with them.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402  (stand-ins for ete3 / Bio / itolapi, the reference on sys.path)
from pastml.tree import read_tree  # noqa: E402
from pastml.utilities.state_simulator import simulate_states  # noqa: E402

N_REP = 20000
SEED = 20231
TREE = os.path.join(mg.DATA, 'Albanian.tree.152tax.tre')
PARAMS = os.path.join(mg.DATA, 'albania_pastml', 'params.character_Country.method_MPPA.model_F81.tab')
COUNTRIES = np.array(['Africa', 'Albania', 'EastEurope', 'Greece', 'WestEurope'])


def tables(tree, character, k):
    nodes = list(tree.traverse('levelorder'))
    hist = np.stack([np.bincount(getattr(n, character), minlength=k) for n in nodes]).astype(np.int64)
    trans = np.zeros((k, k), dtype=np.int64)
    for n in nodes:
        if not n.is_root():
            np.add.at(trans, (getattr(n.up, character), getattr(n, character)), 1)
    return np.array([n.name for n in nodes]), hist, trans


def main():
    tree = read_tree(TREE)
    fs = mg.RForestStats([tree])
    out = dict(n_repetitions=N_REP, seed=SEED)
    f81 = mg.RF81(states=COUNTRIES, forest_stats=fs, parameter_file=PARAMS)
    np.random.seed(SEED)
    simulate_states(tree, f81, 'sim_f81', n_repetitions=N_REP)
    names, hist, trans = tables(tree, 'sim_f81', len(COUNTRIES))
    out.update(names=names, f81_states=COUNTRIES, f81_sf=float(f81.sf), f81_frequencies=np.asarray(f81.frequencies),
               f81_hist=hist, f81_trans=trans)
    jtt = mg.RJTT(forest_stats=fs, sf=float(f81.sf))
    simulate_states(tree, jtt, 'sim_jtt', n_repetitions=N_REP)
    _, hist, trans = tables(tree, 'sim_jtt', len(mg.JTT_STATES))
    out.update(jtt_sf=float(jtt.sf), jtt_hist=hist, jtt_trans=trans)
    path = os.path.join(HERE, 'simulate_albania.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
