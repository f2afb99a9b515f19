#!/usr/bin/env python3
"""
Performance record of the scenario sampler (pml_sample_scenarios) beside the forward simulator (pml_simulate_states) at the
same shapes: a random binary tree of --tips tips (default 262 144), 1024 repetitions, F81 at k = 4 and k = 64 and
CUSTOM_RATES at k = 20.

    scenarios_scale.py [--iters N] [--tips T]     each case: one marginal pass, then per entry point 2 warm-up calls and N timed
                                                  calls; one JSON line per case

A call is timed with HIP events around Engine.sample_scenarios / Engine.simulate_states, so it includes the copy of the
[N, n_rep] states to the host (the same bytes for both entry points); ms are the median over the timed calls.  The line carries
the build digest of the library that ran.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pastml_oracle as orc  # noqa: E402
from pastml_amd import hip  # noqa: E402
from pastml_amd.tree import FlatForest  # noqa: E402

N_REP = 1024
WARMUP = 2
CASES = [('F81', 4), ('F81', 64), ('CUSTOM_RATES', 20)]


def spec_for(kind, k):
    rng = np.random.default_rng(1000 + k)
    if kind == 'F81':
        return dict(kind=hip.KIND_F81, pi=rng.dirichlet(np.ones(k) * 2)), (1.0, 0.0, 1.0)
    pi = rng.dirichlet(np.ones(k) * 3)
    r = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
    d, a, ainv = orc.diagonalise(pi, r + r.T)
    return dict(kind=hip.KIND_EIGEN, pi=pi, d=d, A=a, Ainv=ainv), (1.0, 0.0, 1.0)


def tip_masks(flat, k):
    rng = np.random.default_rng(k)
    m = np.ones((flat.n_nodes, k), dtype=np.int8)
    m[flat.tips] = 0
    m[flat.tips, rng.integers(0, k, size=len(flat.tips))] = 1
    return m


def timed(eng, call, iters):
    for i in range(WARMUP):
        call(i)
    ms = []
    for i in range(iters):
        eng.timer_start()
        call(100 + i)
        ms.append(eng.timer_stop())
    return float(np.median(ms))


def run(flat, kind, k, iters):
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([spec_for(kind, k)])
        eng.set_masks(tip_masks(flat, k)[None])
        eng.bottom_up(True)
        eng.top_down_marginals(posterior=False, lh=False)
        fallen = []
        scen = timed(eng, lambda s: fallen.append(eng.sample_scenarios(N_REP, s)[1]), iters)
        sim = timed(eng, lambda s: eng.simulate_states(N_REP, s), iters)
    print(json.dumps(dict(model=kind, k=k, tips=len(flat.tips), nodes=flat.n_nodes, n_rep=N_REP, iters=iters,
                          sample_scenarios_ms_per_1024=round(scen, 3), simulate_states_ms_per_1024=round(sim, 3),
                          ratio=round(scen / sim, 3), n_fallback=int(sum(fallen)), build_digest=hip.build_digest())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--tips', type=int, default=262144)
    a = ap.parse_args()
    flat = FlatForest.random(a.tips, seed=1, max_arity=2)
    for kind, k in CASES:
        run(flat, kind, k, a.iters)


if __name__ == '__main__':
    main()
