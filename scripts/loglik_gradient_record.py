#!/usr/bin/env python3
"""
Record of the exact gradient of ln L (pml_loglik_gradient): accuracy, cost and the stored Albania optimum.

    loglik_gradient_record.py [--iters N] [--out FILE]

1. The worst error ratios |device - exact| / gross of tests/test_gpu_loglik_gradient.py: the file is run in a child process
   with -s and a time limit and its 'ratio' lines are read; 8 x the worst is the tolerance the tests carry.  If the child ends
   with anything but a pass or plain test failures, the script stops there and starts nothing more on the GPU.
2. The gradient pass next to the marginal pass it follows, 262 144 tips x 32 columns x k = 64 (every column its own
   parameters): 3 warm-up calls and N timed calls (default 20; median [min, max]), HIP events on the context's stream around
   the call -- launches, the call's scratch and the copy of the results included.
3. The HIV1C tree at k = 67, both through hip.Engine, model upload included: one marginal pass + the gradient of one column,
   against one finite-difference round of 69 bottom-up columns (the point and its 68 neighbours at step 1e-8: sf, tau and the
   66 frequency ratios free).
4. The gradient at the stored Albania F81 optimum (tests/golden/albania_F81.npz), projected on the optimiser's bounds.
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

GOLDEN = os.path.join(REPO, 'tests', 'golden')
TESTS_TIME_LIMIT = 300   # seconds for the child that runs the test file (it takes about ten)


def test_ratios():
    run = subprocess.run([sys.executable, '-m', 'pytest', os.path.join('tests', 'test_gpu_loglik_gradient.py'), '-m', 'gpu', '-s',
                          '-q', '-p', 'no:cacheprovider'], cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=TESTS_TIME_LIMIT)
    if run.returncode not in (0, 1):
        # killed, aborted or hung (subprocess.run raises at the time limit): nothing more is started on the GPU after that
        sys.stdout.write(run.stdout[-4000:])
        raise SystemExit('the test file ended with status {}: stopping here'.format(run.returncode))
    worst = dict(rates=(0.0, None), frequencies=(0.0, None), parameters=(0.0, None))
    n = 0
    for line in run.stdout.splitlines():
        m = re.search(r'ratio (.*?): (.*)$', line)
        if not m:
            continue
        n += 1
        for name, value in re.findall(r'(rates|frequencies|parameters) ([0-9.eE+-]+)', m.group(2)):
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


def full_size(iters):
    from pastml_amd import hip, synthetic
    L, k, cols = 18, 64, 32
    flat = synthetic.balanced_forest(L)
    rng = np.random.default_rng(1)
    states = rng.integers(0, k, size=(cols, len(flat.tips))).astype(np.int32)
    states[:, ::17] = -1
    models = [(dict(kind=hip.KIND_F81, pi=np.random.default_rng(1000 + c).dirichlet(np.ones(k) * 2)), (1.0 + 0.1 * c, 0.0, 1.0))
              for c in range(cols)]
    with hip.Engine(flat, cols, k) as eng:
        eng.set_models(models)
        eng.set_tip_states(states)
        eng.marginal_pass(posterior=False, lh=False)
        out = dict(part='full_size', tips=len(flat.tips), nodes=flat.n_nodes, k=k, cols=cols, iters=iters)
        out['marginal_ms'] = timed(eng, lambda: eng.marginal_pass(posterior=False, lh=False), iters)
        out['gradient_ms'] = timed(eng, lambda: eng.loglik_gradient(), iters)
        d_rates, d_pi, n_flat = eng.loglik_gradient()
        out['finite'] = bool(np.isfinite(d_rates).all() and np.isfinite(d_pi).all())
        out['n_flat_max'] = int(n_flat.max())
        out['ratio_gradient_to_marginal'] = out['gradient_ms'][0] / out['marginal_ms'][0]
        # what the pass streams per branch and column: the parent's posterior row and the branch's bottom-up row (a tip's row is
        # read too: every load is issued), 2 x ks x 8 bytes
        gb = 2.0 * 8 * k * flat.n_nodes * cols / 1e9
        out['model_gb'] = gb
        out['model_tb_per_s'] = gb / out['gradient_ms'][0]
    return out


def hiv1c(iters):
    from pastml_amd import hip
    from pastml_amd.annotation import ForestStats
    from pastml_amd.tree import read_tree, get_flat_forest
    nwk = os.path.join(GOLDEN, 'data', 'hiv1c', 'pastml_phyml_tree.nwk')
    flat = get_flat_forest([read_tree(nwk)])
    k, n = 67, 68   # free: sf, tau and k - 1 frequency ratios -- the 69 columns of a finite-difference round of the HIV1C columns
    stats = ForestStats(flat)
    L, nodes = stats.forest_length, stats.num_nodes
    rng = np.random.default_rng(5)
    tips = rng.integers(0, k, size=flat.n_tips)
    pi = rng.dirichlet(np.ones(k) * 5)
    x = np.concatenate(([5.5, 0.1 * stats.avg_nonzero_brlen], pi[:-1] / pi[-1]))
    points = np.repeat(x[None, :], n + 1, axis=0)
    points[np.arange(1, n + 1), np.arange(n)] += 1e-8

    def decode(p):
        ratios = np.concatenate((p[2:], [1.0]))
        return dict(kind=hip.KIND_F81, pi=ratios / ratios.sum()), (float(p[0]), float(p[1]), float(L / (L + p[1] * (nodes - 1))))

    out = dict(part='hiv1c', tips=int(flat.n_tips), nodes=flat.n_nodes, k=k, fd_columns=n + 1, iters=iters)
    with hip.Engine(flat, 1, k) as eng:
        eng.set_tip_states(tips[None, :])

        def exact():
            eng.set_models([decode(x)])
            eng.marginal_pass(posterior=False, lh=False)
            return eng.loglik_gradient()
        out['marginal_plus_gradient_ms'] = timed(eng, exact, iters)

        def marginal_only():
            eng.set_models([decode(x)])
            eng.marginal_pass(posterior=False, lh=False)
        out['marginal_ms'] = timed(eng, marginal_only, iters)
        d_rates, d_pi, n_flat = exact()
        g, tf = d_pi[0], L / (L + x[1] * (nodes - 1))
        exact_x = np.concatenate(([d_rates[0, 0], d_rates[0, 1] - d_rates[0, 2] * tf * tf * (nodes - 1) / L],
                                  (g[:-1] - pi.dot(g)) / (1.0 + x[2:].sum())))
        out['n_flat'] = int(n_flat[0])
    with hip.Engine(flat, n + 1, k) as eng:
        eng.set_tip_states(np.tile(tips, (n + 1, 1)))

        def fd_round():
            eng.set_models([decode(p) for p in points])
            return eng.bottom_up(True)
        out['fd_round_ms'] = timed(eng, fd_round, iters)
        lnl = fd_round()
        fd = (lnl[1:] - lnl[0]) / 1e-8
    out['ratio_exact_to_fd_round'] = out['marginal_plus_gradient_ms'][0] / out['fd_round_ms'][0]
    out['max_abs_fd_minus_exact'] = float(np.abs(fd - exact_x).max())
    out['max_abs_exact'] = float(np.abs(exact_x).max())
    return out


def albania():
    import pandas as pd
    from pastml_amd import ml
    from pastml_amd.annotation import ForestStats, preannotate_forest
    from pastml_amd.models.F81Model import F81Model
    from pastml_amd.tree import read_tree
    zz = np.load(os.path.join(GOLDEN, 'albania_F81.npz'), allow_pickle=False)
    tree = read_tree(os.path.join(GOLDEN, 'data', 'Albanian.tree.152tax.tre'))
    preannotate_forest([tree], df=pd.read_csv(os.path.join(GOLDEN, 'data', 'data.txt'), index_col=0, header=0)[['Country']])
    model = F81Model(states=zz['opt_states'], forest_stats=ForestStats([tree]), sf=float(zz['opt_sf']),
                     frequencies=zz['opt_frequencies'])
    res = ml.loglikelihood_gradient([tree], 'Country', model)
    x, bounds, g = model.get_optimised_parameters(), model.get_bounds(), res['parameters']
    blocked = ((x <= bounds[:, 0]) & (g < 0)) | ((x >= bounds[:, 1]) & (g > 0))   # (ln L is maximised: ascent along +g)
    projected = np.where(blocked, 0.0, g)
    return dict(part='albania_F81_optimum', log_likelihood=res['log_likelihood'], parameter_names=res['parameter_names'],
                x=x.tolist(), gradient=g.tolist(), at_bound=blocked.tolist(), projected_gradient=projected.tolist(),
                max_abs_projected=float(np.abs(projected).max()), n_zero_length_branches=res['n_zero_length_branches'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--parts', type=str, default='tests,full,hiv1c,albania')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    parts = dict(tests=test_ratios, full=lambda: full_size(args.iters), hiv1c=lambda: hiv1c(args.iters), albania=albania)
    lines = []
    for name in args.parts.split(','):
        lines.append(json.dumps(parts[name]()))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
