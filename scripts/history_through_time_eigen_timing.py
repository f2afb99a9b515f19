#!/usr/bin/env python3
"""
Cost of the dwell times, jumps and lineages per time interval of the eigen models (pml_history_through_time_eigen) next to
pml_expected_history_eigen on the same context, the marginal pass excluded.

    history_through_time_eigen_timing.py [--iters N] [--levels L] [--cols C] [--ks 20,61] [--bins 1,16] [--out FILE]

A balanced tree of 65 536 tips x 4 characters (every column its own reversible model), at k = 20 and k = 61; node times are root
distances, the M bins are equal and cover the tree.  In one process, on one marginal pass, the calls are timed in turn, round
after round (so that a drift of the machine touches all alike): pml_expected_history_eigen with times and jumps, then
pml_history_through_time_eigen with everything for every M, and with times only at the largest M.  3 warm-up rounds, then N timed
rounds (default 10; median [min, max]); HIP events on the context's stream around each call -- the segment plan on the host, its
upload, the launches, the call's scratch and the copy of the results included.

The byte model: per branch and column 2 k doubles streamed in and 3 k staged, as in pml_expected_history_eigen; per
segment and column 3 k doubles read from the branch's staged vectors, 3 k written and read back once per tile of pairs; per piece
and column a k x k partial written and read; 3 M k^2 doubles per column for W_m, its first product and the jumps.  At M = 1 the
segments are the branches: the whole-tree entry's bytes plus the segments' 6 k.
One JSON line per k; --out writes them to a file.  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def measure(k, levels, cols, iters, bins, warmup=3):
    from oracle import pastml_oracle as orc
    from pastml_amd import hip, synthetic
    from pastml_amd.tree import annotate_dates
    flat = synthetic.balanced_forest(levels)
    rng = np.random.default_rng(k)
    states = rng.integers(0, k, size=(cols, len(flat.tips))).astype(np.int32)
    states[:, ::17] = -1
    models = []
    for c in range(cols):
        pi = rng.dirichlet(np.ones(k) * 2)
        R = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
        d, a, ainv = orc.diagonalise(pi, R + R.T)
        models.append((dict(kind=hip.KIND_EIGEN, pi=pi, d=d, A=a, Ainv=ainv), (1.0 + 0.1 * c, 0.0, 1.0)))
    t = annotate_dates(flat)
    out = dict(k=k, tips=len(flat.tips), nodes=flat.n_nodes, cols=cols, iters=iters, warmup=warmup, bins=list(bins))
    with hip.Engine(flat, cols, k) as eng:
        eng.set_models(models)
        eng.set_tip_states(states)
        eng.marginal_pass(posterior=False, lh=False)
        bounds = {M: np.linspace(t.min(), t.max(), M + 1) for M in bins}
        calls = dict(expected_history_eigen=lambda: eng.expected_history_eigen(jumps=True, branch_jumps=False))
        for M in bins:
            calls['through_time_M{}'.format(M)] = lambda M=M: eng.history_through_time_eigen(t, bounds[M])
        calls['through_time_M{}_times_only'.format(bins[-1])] = lambda: eng.history_through_time_eigen(
            t, bounds[bins[-1]], jumps=False, lineages=False)
        ms = {name: [] for name in calls}
        for r in range(warmup + iters):
            for name, call in calls.items():
                eng.timer_start()
                call()
                elapsed = eng.timer_stop()
                if r >= warmup:
                    ms[name].append(elapsed)
        whole_times, whole_jumps, _ = eng.expected_history_eigen()
        length = float(flat.dist[flat.parent >= 0].sum())
        for M in bins:
            times, jumps, lineages = eng.history_through_time_eigen(t, bounds[M])
            segments = int(sum((np.minimum(t, hi) > np.maximum(t[np.maximum(flat.parent, 0)], lo))[flat.parent >= 0].sum()
                               for lo, hi in zip(bounds[M][:-1], bounds[M][1:])))
            out['M{}_segments'.format(M)] = segments
            out['M{}_finite'.format(M)] = bool(np.isfinite(times).all() and np.isfinite(jumps).all() and np.isfinite(lineages).all())
            out['M{}_worst_times_against_expected_history_eigen'.format(M)] = float(
                (np.abs(times.sum(axis=1) - whole_times) / whole_times.max(axis=1, keepdims=True)).max())
            out['M{}_worst_jumps_against_expected_history_eigen'.format(M)] = float(
                (np.abs(jumps.sum(axis=1) - whole_jumps) / whole_jumps.max(axis=(1, 2), keepdims=True)).max())
            out['M{}_worst_length'.format(M)] = float(np.abs(times.sum(axis=(1, 2)) - length).max() / length)
            pieces = segments // 512 + M
            out['M{}_model_gb'.format(M)] = 8.0 * cols * (5 * k * flat.n_nodes + 9 * k * segments + 2 * pieces * k * k + 6 * M * k * k) / 1e9
    for name, values in ms.items():
        out[name + '_ms'] = (float(np.median(values)), float(np.min(values)), float(np.max(values)))
    for M in bins:
        out['ratio_M{}_to_expected_history_eigen'.format(M)] = (out['through_time_M{}_ms'.format(M)][0] /
                                                                 out['expected_history_eigen_ms'][0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--levels', type=int, default=16)
    ap.add_argument('--cols', type=int, default=4)
    ap.add_argument('--ks', type=str, default='20,61')
    ap.add_argument('--bins', type=str, default='1,16')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    bins = [int(x) for x in args.bins.split(',')]
    lines = []
    for k in (int(x) for x in args.ks.split(',')):
        lines.append(json.dumps(measure(k, args.levels, args.cols, args.iters, bins)))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
