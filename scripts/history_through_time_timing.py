#!/usr/bin/env python3
"""
Cost of the dwell times, jumps and lineages per time interval (pml_history_through_time) next to pml_expected_history on the same
context, the marginal pass excluded.

    history_through_time_timing.py [--iters N] [--tips T] [--cols C] [--ks 4,64] [--bins 1,16,256] [--out FILE]

A random binary tree of 65 536 tips x 32 characters (every column its own parameters), at k = 4 and k = 64; node times are root
distances, the M bins are equal and cover the tree.  In one process, on one marginal pass, the calls are timed in turn, round
after round (so that a drift of the machine touches all alike): pml_expected_history with times and jumps, then
pml_history_through_time with everything for every M, and with times only at the largest M.  3 warm-up rounds, then N timed
rounds (default 10; median [min, max]); HIP events on the context's stream around each call -- the segment plan on the host, its
upload, the launches, the call's scratch and the copy of the results included.

The byte model: per segment and column the parent's posterior row and the branch's bottom-up row, 2 k doubles, in
the segment pass and again in the jump product, plus 24 bytes staged and 40 bytes of plan; per non-empty bin and column at
least one k x k partial written and read; M k^2 doubles per column copied to the host.  At M = 1 the segments are the branches:
the same bytes as pml_expected_history.
One JSON line per k; --out writes them to a file.  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def measure(k, n_tips, cols, iters, bins, warmup=3):
    from pastml_amd import hip
    from pastml_amd.tree import FlatForest, annotate_dates
    flat = FlatForest.random(n_tips, seed=17, max_arity=2, zero_frac=0.0, n_trees=1)
    rng = np.random.default_rng(1)
    states = rng.integers(0, k, size=(cols, len(flat.tips))).astype(np.int32)
    states[:, ::17] = -1
    models = [(dict(kind=hip.KIND_F81, pi=np.random.default_rng(1000 + c).dirichlet(np.ones(k) * 2)), (1.0 + 0.1 * c, 0.0, 1.0))
              for c in range(cols)]
    t = annotate_dates(flat)
    out = dict(k=k, tips=len(flat.tips), nodes=flat.n_nodes, cols=cols, iters=iters, warmup=warmup, bins=list(bins))
    with hip.Engine(flat, cols, k) as eng:
        eng.set_models(models)
        eng.set_tip_states(states)
        eng.marginal_pass(posterior=False, lh=False)
        bounds = {M: np.linspace(t.min(), t.max(), M + 1) for M in bins}
        calls = dict(expected_history=lambda: eng.expected_history(jumps=True, branch_jumps=False))
        for M in bins:
            calls['through_time_M{}'.format(M)] = lambda M=M: eng.history_through_time(t, bounds[M])
        calls['through_time_M{}_times_only'.format(bins[-1])] = lambda: eng.history_through_time(t, bounds[bins[-1]], jumps=False,
                                                                                                lineages=False)
        ms = {name: [] for name in calls}
        for r in range(warmup + iters):
            for name, call in calls.items():
                eng.timer_start()
                call()
                elapsed = eng.timer_stop()
                if r >= warmup:
                    ms[name].append(elapsed)
        whole_times, whole_jumps, _ = eng.expected_history()
        length = float(flat.dist[flat.parent >= 0].sum())
        for M in bins:
            times, jumps, lineages = eng.history_through_time(t, bounds[M])
            segments = int(sum((np.minimum(t, hi) > np.maximum(t[np.maximum(flat.parent, 0)], lo))[flat.parent >= 0].sum()
                               for lo, hi in zip(bounds[M][:-1], bounds[M][1:])))
            out['M{}_segments'.format(M)] = segments
            out['M{}_worst_times_against_expected_history'.format(M)] = float(
                (np.abs(times.sum(axis=1) - whole_times) / whole_times).max())
            out['M{}_worst_jumps_against_expected_history'.format(M)] = float(
                np.nanmax(np.abs(jumps.sum(axis=1) - whole_jumps)[whole_jumps > 0] / whole_jumps[whole_jumps > 0]))
            out['M{}_worst_length'.format(M)] = float(np.abs(times.sum(axis=(1, 2)) - length).max() / length)
            out['M{}_model_gb'.format(M)] = (segments * cols * (2 * 2 * 8 * k + 2 * 24 + 40) + 3 * 8.0 * M * k * k * cols) / 1e9
    for name, values in ms.items():
        out[name + '_ms'] = (float(np.median(values)), float(np.min(values)), float(np.max(values)))
    for M in bins:
        out['ratio_M{}_to_expected_history'.format(M)] = out['through_time_M{}_ms'.format(M)][0] / out['expected_history_ms'][0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--tips', type=int, default=65536)
    ap.add_argument('--cols', type=int, default=32)
    ap.add_argument('--ks', type=str, default='4,64')
    ap.add_argument('--bins', type=str, default='1,16,256')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    bins = [int(x) for x in args.bins.split(',')]
    lines = []
    for k in (int(x) for x in args.ks.split(',')):
        lines.append(json.dumps(measure(k, args.tips, args.cols, args.iters, bins)))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
