#!/usr/bin/env python3
"""
Record of the exact expected history of the eigen models (pml_expected_history_eigen): accuracy and cost.

    expected_history_eigen_record.py [--iters N] [--parts tests,timing] [--out FILE]

1. The worst error ratios |device - exact| / (largest exact entry) of tests/test_gpu_expected_history_eigen.py: the file is run
   in a child process with -s and a time limit and its 'ratio' lines are read; 8 x the worst is the tolerance the tests carry.
   If the child ends with anything but a pass or plain test failures, the script stops there and starts nothing more on the GPU.
2. The call next to the marginal pass it follows and to pml_expected_counts on the same context: a balanced tree of 65 536 tips
   x 4 characters (each its own model and rates) at k = 20 and k = 61; 3 warm-up calls and N timed calls (default 10; median
   [min, max]), HIP events on the context's stream around the call -- launches, the call's scratch and the copy of the results
   included.
One JSON line per part; --out writes them to a file.  No time is asserted anywhere.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

TESTS_TIME_LIMIT = 600   # seconds for the child that runs the test file (it takes about one minute)


def test_ratios():
    run = subprocess.run([sys.executable, '-m', 'pytest', os.path.join('tests', 'test_gpu_expected_history_eigen.py'), '-m', 'gpu',
                          '-s', '-q', '-p', 'no:cacheprovider'], cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=TESTS_TIME_LIMIT)
    if run.returncode not in (0, 1):
        # killed, aborted or hung (subprocess.run raises at the time limit): nothing more is started on the GPU after that
        sys.stdout.write(run.stdout[-4000:])
        raise SystemExit('the test file ended with status {}: stopping here'.format(run.returncode))
    worst = dict(times=(0.0, None), jumps=(0.0, None), branch_jumps=(0.0, None))
    n = 0
    for line in run.stdout.splitlines():
        m = re.search(r'ratio (.*?): (.*)$', line)
        if not m:
            continue
        n += 1
        for name, value in re.findall(r'(times|jumps|branch_jumps) ([0-9.eE+-]+)', m.group(2)):
            if float(value) > worst[name][0]:
                worst[name] = (float(value), m.group(1))
    top = max(v[0] for v in worst.values())
    return dict(part='test_ratios', pytest_exit=run.returncode, summary=run.stdout.strip().splitlines()[-1], cases=n, worst=worst,
                worst_ratio=top, tolerance_8x=8 * top)


def timed(eng, call, iters, warmup=3):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(iters):
        eng.timer_start()
        call()
        ms.append(eng.timer_stop())
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def timing(iters):
    from pastml_amd import hip, synthetic
    from oracle import pastml_oracle as orc
    L, cols = 16, 4
    flat = synthetic.balanced_forest(L)
    lines = []
    for k in (20, 61):
        rng = np.random.default_rng(k)
        states = rng.integers(0, k, size=(cols, len(flat.tips))).astype(np.int32)
        states[:, ::17] = -1
        models = []
        for c in range(cols):
            pi = rng.dirichlet(np.ones(k) * 2)
            R = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
            d, a, ainv = orc.diagonalise(pi, R + R.T)
            models.append((dict(kind=hip.KIND_EIGEN, pi=pi, d=d, A=a, Ainv=ainv), (1.0 + 0.1 * c, 0.0, 1.0)))
        with hip.Engine(flat, cols, k) as eng:
            eng.set_models(models)
            eng.set_tip_states(states)
            eng.marginal_pass(posterior=False, lh=False)
            out = dict(part='timing', tips=len(flat.tips), nodes=flat.n_nodes, k=k, cols=cols, iters=iters)
            out['marginal_ms'] = timed(eng, lambda: eng.marginal_pass(posterior=False, lh=False), iters)
            out['history_eigen_ms'] = timed(eng, lambda: eng.expected_history_eigen(), iters)
            out['history_eigen_times_only_ms'] = timed(eng, lambda: eng.expected_history_eigen(jumps=False), iters)
            out['history_eigen_all_ms'] = timed(eng, lambda: eng.expected_history_eigen(branch_jumps=True), iters)
            times, jumps, _ = eng.expected_history_eigen()
            out['finite'] = bool(np.isfinite(times).all() and np.isfinite(jumps).all())
            out['I1_rel'] = float(np.abs(times.sum(axis=1) / flat.dist[flat.parent >= 0].sum() - 1).max())
            out['expected_counts_ms'] = timed(eng, lambda: eng.expected_counts(), iters)   # (builds the P(t) batch first)
            out['ratio_history_to_marginal'] = out['history_eigen_ms'][0] / out['marginal_ms'][0]
            out['ratio_history_to_counts'] = out['history_eigen_ms'][0] / out['expected_counts_ms'][0]
            # streamed in per branch and column: v_n and q_p (2 ks doubles); staged and read back once per tile of pairs: E, r, l
            out['model_gb_in'] = 2.0 * 8 * k * flat.n_nodes * cols / 1e9
            out['model_gb_staged'] = 3.0 * 8 * k * flat.n_nodes * cols / 1e9
        lines.append(out)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--parts', type=str, default='tests,timing')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    parts = dict(tests=lambda: [test_ratios()], timing=lambda: timing(args.iters))
    lines = []
    for name in args.parts.split(','):
        for record in parts[name]():
            lines.append(json.dumps(record))
            print(lines[-1], flush=True)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
