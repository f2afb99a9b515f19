#!/usr/bin/env python3
"""
Performance record of the exact expected transition counts (pml_expected_counts).

    expected_counts_scale.py [--iters N] [--out FILE]

Per case: the context is built, the marginal pass run, then 3 warm-up calls and N timed calls (default 20, the median is
reported) of
    expected   Engine.expected_counts() over all columns: HIP events on the context's stream around the call -- the three
               launches, the allocation and release of the call's scratch and the copy of the [cols, k, k] result
    marginal   Engine.marginal_pass(posterior=False, lh=False) of the same context, the yardstick
    sampled    Engine.marginal_counts(1000 repetitions) of column 0 -- the sampler is untouched by this feature, so this
               library's is the parent commit's; one column, as it serves one column per call
One JSON line per case and a table at the end (median [min, max]); --out writes both to a file.  No time is asserted anywhere.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pastml_oracle as orc  # noqa: E402
from pastml_amd import hip, synthetic  # noqa: E402

CASES = [
    dict(name='f81_k4', kind='F81', k=4, levels=18, cols=32),
    dict(name='f81_k64', kind='F81', k=64, levels=18, cols=32),
    dict(name='eigen_k61', kind='EIGEN', k=61, levels=16, cols=4),
]


def model_of(kind, k, seed):
    rng = np.random.default_rng(1000 + seed)
    rates = (1.0 + 0.1 * seed, 0.0, 1.0)
    if kind == 'F81':
        return dict(kind=hip.KIND_F81, pi=rng.dirichlet(np.ones(k) * 2)), rates
    pi = rng.dirichlet(np.ones(k) * 3)
    r = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
    d, a, ainv = orc.diagonalise(pi, r + r.T)
    return dict(kind=hip.KIND_EIGEN, pi=pi, d=d, A=a, Ainv=ainv), rates


def timed(eng, call, iters, warmup=3):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(iters):
        eng.timer_start()
        call()
        ms.append(eng.timer_stop())
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def run_case(case, iters):
    flat = synthetic.balanced_forest(case['levels'])
    k, cols = case['k'], case['cols']
    rng = np.random.default_rng(1)
    states = rng.integers(0, k, size=(cols, len(flat.tips))).astype(np.int32)
    with hip.Engine(flat, cols, k) as eng:
        eng.set_models([model_of(case['kind'], k, c) for c in range(cols)])
        eng.set_tip_states(states)
        eng.marginal_pass(posterior=False, lh=False)
        out = dict(case=case['name'], tips=len(flat.tips), nodes=flat.n_nodes, k=k, cols=cols, iters=iters)
        out['marginal_ms'] = timed(eng, lambda: eng.marginal_pass(posterior=False, lh=False), iters)
        out['expected_ms'] = timed(eng, lambda: eng.expected_counts(), iters)
        if k <= 256:
            out['sampled_1000_one_column_ms'] = timed(eng, lambda: eng.marginal_counts(1000, seed=7, col=0), max(3, iters // 4), 1)
        counts = eng.expected_counts()
        out['finite'] = bool(np.isfinite(counts).all())
        out['ratio_expected_to_marginal'] = out['expected_ms'][0] / out['marginal_ms'][0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--cases', type=str, default=','.join(c['name'] for c in CASES))
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    lines = []
    for case in CASES:
        if case['name'] not in args.cases.split(','):
            continue
        res = run_case(case, args.iters)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    table = ['case        tips     cols  k    marginal ms              expected ms              expected/marginal  sampled, 1 column, ms']
    fmt = lambda t: '{:7.3f} [{:.3f}, {:.3f}]'.format(*t)   # noqa: E731   median [min, max]
    for r in map(json.loads, lines):
        table.append('{:10s}  {:7d}  {:4d}  {:3d}  {}  {}  {:6.2f}             {}'.format(
            r['case'], r['tips'], r['cols'], r['k'], fmt(r['marginal_ms']), fmt(r['expected_ms']),
            r['ratio_expected_to_marginal'], fmt(r['sampled_1000_one_column_ms']) if 'sampled_1000_one_column_ms' in r else '-'))
    print('\n'.join(table), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines + [''] + table) + '\n')


if __name__ == '__main__':
    main()
