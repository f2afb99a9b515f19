#!/usr/bin/env python3
"""
What polytomy resolution costs at scale: acr() on a random 100 000-tip forest with polytomies (max arity 8) x 16
characters, k = 20, F81 MPPA at fixed parameters, with resolve_polytomies off and on, each in one process.

    timeout -k 10 900 python3 scripts/polytomy_scale.py [OUT]      (default OUT: profiles/polytomy_scale.txt)

Reported per run: the resolve / unresolve rounds and the wall seconds split into
  editing      resolve_trees / unresolve_trees without their re-flattening (grouping, new and removed nodes)
  flatten      re-flattening the edited forest (pastml_amd.tree._reflatten: FlatForest.from_trees + columns)
  run_tasks    the batched likelihood path per round: tree upload (schedule planning included), device sweeps
               (one evaluation, joint pass, marginal pass, selections) and the per-group host work around them
  assembly     the rest of acr(): plan, frequencies, restored annotations, forest statistics, result dictionaries
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

N_TIPS, K, N_CHARS, SWITCH = 100000, 20, 16, 0.6


def forest_and_table():
    from pastml_amd.tree import FlatForest
    flat = FlatForest.random(N_TIPS, seed=5, max_arity=8, zero_frac=0.05)
    rng = np.random.default_rng(6)
    table = {}
    states = np.array(['s{:02d}'.format(i) for i in range(K)])
    for c in range(N_CHARS):
        # a walk down the levels: a state changes on a branch with probability 1 - exp(-SWITCH * dist * 10)
        s = np.zeros(flat.n_nodes, dtype=np.int64)
        s[flat.roots] = rng.integers(K, size=len(flat.roots))
        for d in range(1, flat.n_td_levels):
            a, b = flat.td_offsets[d], flat.td_offsets[d + 1]
            s[a:b] = s[flat.parent[a:b]]
            change = rng.random(b - a) < 1 - np.exp(-SWITCH * 10 * flat.dist[a:b])
            s[a:b][change] = rng.integers(K, size=int(change.sum()))
        table['c{}'.format(c)] = states[s[flat.tips]]
    names = [flat.nodes[i].name for i in flat.tips]
    return [flat.nodes[r] for r in flat.roots], pd.DataFrame(table, index=names), states


def run(resolve):
    from pastml_amd import acr as acr_module, batch, tree
    roots, df, states = forest_and_table()
    freqs = np.linspace(2, 1, K)
    freqs /= freqs.sum()
    params = {c: dict({'scaling_factor': 4.0}, **dict(zip(states, freqs))) for c in df.columns}
    t = dict(editing=0.0, flatten=0.0, run_tasks=0.0)
    rounds = dict(resolve=[], unresolve=[], run_tasks=0)

    def timed(fn, key, log=None):
        def wrapper(*args, **kwargs):
            t0 = time.perf_counter()
            out = fn(*args, **kwargs)
            t[key] += time.perf_counter() - t0
            if log is not None:
                rounds[log].append(out)
            return out
        return wrapper

    real_run_tasks = batch.run_tasks

    def run_tasks(*args, **kwargs):
        rounds['run_tasks'] += 1
        return timed(real_run_tasks, 'run_tasks')(*args, **kwargs)

    acr_module.resolve_trees = timed(tree.resolve_trees, 'editing', 'resolve')
    acr_module.unresolve_trees = timed(tree.unresolve_trees, 'editing', 'unresolve')
    tree._reflatten = timed(tree._reflatten, 'flatten')
    batch.run_tasks = run_tasks
    np.random.seed(1)
    t0 = time.perf_counter()
    res = acr_module.acr(roots, df, prediction_method='MPPA', model='F81', column2parameters=params,
                         resolve_polytomies=resolve)
    total = time.perf_counter() - t0
    t['editing'] -= t['flatten']
    n_nodes = sum(1 for r in roots for _ in r.traverse())
    lnl = sum(r['log_likelihood'] for r in res)
    return ('resolve_polytomies={}: {} nodes after, total ln L {:.6f}\n'
            '  rounds: resolve_trees -> {}, unresolve_trees -> {}, run_tasks calls {}\n'
            '  wall s: total {:.3f} | editing {:.3f} | flatten {:.3f} | run_tasks {:.3f} | assembly {:.3f}\n'
            .format(resolve, n_nodes, lnl, rounds['resolve'], rounds['unresolve'], rounds['run_tasks'], total,
                    t['editing'], t['flatten'], t['run_tasks'], total - t['editing'] - t['flatten'] - t['run_tasks']))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, 'profiles', 'polytomy_scale.txt')
    if len(sys.argv) > 2:   # one measurement per process: the child prints its block
        sys.stdout.write(run(sys.argv[2] == 'on'))
        return
    import subprocess
    text = ['polytomy_scale: {} tips, max arity 8, {} characters x k = {}, F81 MPPA at fixed parameters\n'
            .format(N_TIPS, N_CHARS, K)]
    for mode in ('off', 'on'):
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), out, mode], capture_output=True, text=True,
                              timeout=800)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(proc.returncode)
        text.append(proc.stdout)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        f.writelines(text)
    sys.stdout.writelines(text)


if __name__ == '__main__':
    main()
