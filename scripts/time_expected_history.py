#!/usr/bin/env python3
"""
Cost of the exact expected dwell times and Markov jumps (pml_expected_history) next to the passes it is modelled on.

    time_expected_history.py [--iters N] [--tips T] [--cols C] [--out FILE]

A random binary tree of 262 144 tips x 32 characters (every column its own parameters), at k = 4 and k = 64.  In one process, on
one marginal pass, the calls are timed in turn, round after round (so that a drift of the machine touches all alike):
pml_loglik_gradient, pml_expected_counts, pml_expected_history with times only, with times and jumps, and with everything
(branch_jumps too: N doubles per column copied to the host, where the other outputs are k or k^2).
3 warm-up rounds, then N timed rounds (default 20; median [min, max]); HIP events on the context's stream around each call --
launches, the call's scratch and the copy of the results included.

The byte model of the branch pass: per branch and column the parent's posterior row and the branch's bottom-up row, 2 k doubles
(a tip's row is read too: every load is issued).  The share of the HBM peak is that model over the call's time over 8 TB/s: a
whole-call figure, not a kernel's.
One JSON line per k; --out writes them to a file.  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_TB_PER_S = 8.0


def measure(k, n_tips, cols, iters, warmup=3):
    from pastml_amd import hip
    from pastml_amd.tree import FlatForest
    flat = FlatForest.random(n_tips, seed=17, max_arity=2, zero_frac=0.0, n_trees=1)
    rng = np.random.default_rng(1)
    states = rng.integers(0, k, size=(cols, len(flat.tips))).astype(np.int32)
    states[:, ::17] = -1
    models = [(dict(kind=hip.KIND_F81, pi=np.random.default_rng(1000 + c).dirichlet(np.ones(k) * 2)), (1.0 + 0.1 * c, 0.0, 1.0))
              for c in range(cols)]
    out = dict(k=k, tips=len(flat.tips), nodes=flat.n_nodes, cols=cols, iters=iters, warmup=warmup)
    with hip.Engine(flat, cols, k) as eng:
        eng.set_models(models)
        eng.set_tip_states(states)
        eng.marginal_pass(posterior=False, lh=False)
        calls = dict(gradient=lambda: eng.loglik_gradient(),
                     expected_counts=lambda: eng.expected_counts(),
                     history_times_only=lambda: eng.expected_history(jumps=False, branch_jumps=False),
                     history_times_and_jumps=lambda: eng.expected_history(jumps=True, branch_jumps=False),
                     history_everything=lambda: eng.expected_history(jumps=True, branch_jumps=True))
        ms = {name: [] for name in calls}
        for r in range(warmup + iters):
            for name, call in calls.items():
                eng.timer_start()
                call()
                t = eng.timer_stop()
                if r >= warmup:
                    ms[name].append(t)
        times, jumps, branch = eng.expected_history(jumps=True, branch_jumps=True)
        out['finite'] = bool(np.isfinite(times).all() and np.isfinite(jumps).all() and np.isfinite(branch).all())
        length = float(flat.dist[flat.parent >= 0].sum())
        out['worst_I1'] = float(np.abs(times.sum(axis=1) - length).max() / length)
        out['worst_I3'] = float(np.abs(branch.sum(axis=1) - jumps.sum(axis=(1, 2))).max() / jumps.sum(axis=(1, 2)).min())
    for name, values in ms.items():
        out[name + '_ms'] = (float(np.median(values)), float(np.min(values)), float(np.max(values)))
    out['bytes_per_branch_and_column'] = 2 * 8 * k
    gb = 2.0 * 8 * k * flat.n_nodes * cols / 1e9
    out['model_gb'] = gb
    for name in ms:
        out[name + '_model_tb_per_s'] = gb / out[name + '_ms'][0]
        out[name + '_share_of_hbm_peak'] = gb / out[name + '_ms'][0] / HBM_PEAK_TB_PER_S
    out['ratio_times_only_to_gradient'] = out['history_times_only_ms'][0] / out['gradient_ms'][0]
    out['ratio_everything_to_expected_counts'] = out['history_everything_ms'][0] / out['expected_counts_ms'][0]
    out['ratio_times_and_jumps_to_expected_counts'] = out['history_times_and_jumps_ms'][0] / out['expected_counts_ms'][0]
    out['branch_jumps_mb_to_host'] = 8.0 * flat.n_nodes * cols / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--tips', type=int, default=262144)
    ap.add_argument('--cols', type=int, default=32)
    ap.add_argument('--ks', type=str, default='4,64')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    lines = []
    for k in (int(x) for x in args.ks.split(',')):
        lines.append(json.dumps(measure(k, args.tips, args.cols, args.iters)))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
