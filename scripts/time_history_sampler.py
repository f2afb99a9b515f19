#!/usr/bin/env python3
"""
Cost of the history sampler (pml_sample_histories) next to the scenario sampler it builds on (pml_sample_scenarios), on the same
context: a random binary tree of --tips tips (default 65 536), 1024 repetitions, F81 at k = 4 and k = 64, branches of
x = mu t' up to 0.4 (mostly well below 1).

    time_history_sampler.py [--iters N] [--tips T] [--out FILE]     each case: one marginal pass, then per entry 2 warm-up calls
                                                                    and N timed calls; one JSON line per case

A call is timed with HIP events around the Engine method, so it includes what the call copies to the host: the [N, n_rep]
states for sample_scenarios and for the `with states` line, the times (and jumps) otherwise.  ms are the median over the timed
calls; the ratios are over sample_scenarios.  The line carries the build digest of the library that ran.
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


def tip_masks(flat, k):
    rng = np.random.default_rng(k)
    m = np.ones((flat.n_nodes, k), dtype=np.int8)
    m[flat.tips] = 0
    m[flat.tips, rng.integers(0, k, size=len(flat.tips))] = 1
    return m


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


def run(flat, k, iters):
    pi = np.random.default_rng(1000 + k).dirichlet(np.ones(k) * 2)
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([(dict(kind=hip.KIND_F81, pi=pi), (1.0, 0.0, 1.0))])
        eng.set_masks(tip_masks(flat, k)[None])
        eng.bottom_up(True)
        eng.top_down_marginals(posterior=False, lh=False)
        scen = timed(eng, lambda s: eng.sample_scenarios(N_REP, s), iters)
        plain = timed(eng, lambda s: eng.sample_histories(N_REP, s, jumps=False, states=False), iters)
        jumps = timed(eng, lambda s: eng.sample_histories(N_REP, s, jumps=True, states=False), iters)
        full = timed(eng, lambda s: eng.sample_histories(N_REP, s, jumps=True, states=True), iters)
        out = eng.sample_histories(N_REP, 7, jumps=True, states=False)
    mean_jumps = float(out[2].sum()) / N_REP
    min_max, spread[:] = list(spread), []
    return dict(k=k, tips=len(flat.tips), nodes=flat.n_nodes, n_rep=N_REP, iters=iters,
                sample_scenarios_ms=round(scen, 3), sample_histories_times_ms=round(plain, 3),
                sample_histories_times_jumps_ms=round(jumps, 3), sample_histories_with_states_ms=round(full, 3),
                ratio_times=round(plain / scen, 3), ratio_times_jumps=round(jumps / scen, 3),
                ratio_with_states=round(full / scen, 3), jumps_per_repetition=round(mean_jumps, 1), min_max_ms=min_max,
                build_digest=hip.build_digest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--tips', type=int, default=65536)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    flat = FlatForest.random(a.tips, seed=1, max_arity=2)
    lines = []
    for k in KS:
        lines.append(json.dumps(run(flat, k, a.iters)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
