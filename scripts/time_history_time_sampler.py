#!/usr/bin/env python3
"""
Cost of the history sampler per time interval (pml_sample_histories_through_time) next to the whole-tree sampler it cuts
(pml_sample_histories), on the same context: a random binary tree of --tips tips (default 65 536) dated by its root distances,
1024 repetitions, F81 at k = 4 and k = 64, branches of x = mu t' up to 0.4 (mostly well below 1); M = 1 and M = 16 equal bins
that cover the tree.

    time_history_time_sampler.py [--iters N] [--tips T] [--out FILE]   each case: one marginal pass, then per entry 2 warm-up
                                                                       calls and N timed calls; one JSON line per case

A call is timed with HIP events around the Engine method, so it includes the host's segment plan, the call's scratch and what
the call copies to the host (times [R, M, k], jumps [R, M, k, k], lineages [R, M + 1, k]; never the states).  ms are the median
over the timed calls; the ratios of M = 1 are over sample_histories with jumps, those of M = 16 over M = 1.  The line carries
the build digest of the library that ran.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pastml_amd import hip  # noqa: E402
from pastml_amd.tree import FlatForest  # noqa: E402

N_REP = 1024
WARMUP = 2
KS = (4, 64)
BINS = (1, 16)


def tip_masks(flat, k):
    rng = np.random.default_rng(k)
    m = np.ones((flat.n_nodes, k), dtype=np.int8)
    m[flat.tips] = 0
    m[flat.tips, rng.integers(0, k, size=len(flat.tips))] = 1
    return m


def root_distance(flat):
    t = np.zeros(flat.n_nodes)
    for n in range(flat.n_nodes):   # (parents come first)
        if flat.parent[n] >= 0:
            t[n] = t[flat.parent[n]] + flat.dist[n]
    return t


spread = []   # (min, max) of every timed entry, in the order of the line's ms fields


def timed(eng, call, iters):
    for i in range(WARMUP):
        call(i)
    ms = []
    for i in range(iters):
        eng.timer_start()
        call(100 + i)
        ms.append(eng.timer_stop())
    spread.append((round(min(ms), 3), round(max(ms), 3)))
    return float(np.median(ms))


def run(flat, t, k, iters):
    pi = np.random.default_rng(1000 + k).dirichlet(np.ones(k) * 2)
    span = t.max() - t.min()
    line = dict(k=k, tips=len(flat.tips), nodes=flat.n_nodes, n_rep=N_REP, iters=iters)
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([(dict(kind=hip.KIND_F81, pi=pi), (1.0, 0.0, 1.0))])
        eng.set_masks(tip_masks(flat, k)[None])
        eng.bottom_up(True)
        eng.top_down_marginals(posterior=False, lh=False)
        whole = timed(eng, lambda s: eng.sample_histories(N_REP, s, jumps=True, states=False), iters)
        line['sample_histories_times_jumps_ms'] = round(whole, 3)
        ms = {}
        for M in BINS:
            T = t.min() - 0.01 * span + 1.02 * span * np.arange(M + 1) / M
            ms[M, 'times'] = timed(eng, lambda s: eng.sample_histories_through_time(t, T, N_REP, s, jumps=False, lineages=False,
                                                                                    states=False), iters)
            ms[M, 'all'] = timed(eng, lambda s: eng.sample_histories_through_time(t, T, N_REP, s, states=False), iters)
            line['M{}_times_ms'.format(M)] = round(ms[M, 'times'], 3)
            line['M{}_times_jumps_lineages_ms'.format(M)] = round(ms[M, 'all'], 3)
            out = eng.sample_histories_through_time(t, T, N_REP, 7, states=False)
            line['M{}_jumps_per_repetition'.format(M)] = round(float(out[2].sum()) / N_REP, 1)
            line['M{}_segments'.format(M)] = int(sum((np.minimum(T[m + 1], t[flat.parent >= 0]) >
                                                      np.maximum(T[m], t[flat.parent[flat.parent >= 0]])).sum() for m in range(M)))
    line['ratio_M1_over_sample_histories'] = round(ms[1, 'all'] / whole, 3)
    line['ratio_M16_over_M1'] = round(ms[16, 'all'] / ms[1, 'all'], 3)
    line['ratio_M16_over_M1_times_only'] = round(ms[16, 'times'] / ms[1, 'times'], 3)
    line['min_max_ms'], spread[:] = list(spread), []
    line['build_digest'] = hip.build_digest()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--tips', type=int, default=65536)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    flat = FlatForest.random(a.tips, seed=1, max_arity=2)
    t = root_distance(flat)
    lines = []
    for k in KS:
        lines.append(json.dumps(run(flat, t, k, a.iters)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
