#!/usr/bin/env python3
"""
Record of the bits of the four exact history entries (pml_expected_history, pml_expected_history_eigen, pml_history_through_time,
pml_history_through_time_eigen): one line per case and output array with the array's sha256, to be compared between two builds
of the library on the same machine -- a refactoring of these kernels that keeps every statement and the order of every sum
leaves the file byte-identical.

    history_bits_record.py [--out FILE]

The cases run in one child process with a time limit; if it ends with anything but 0, the script stops there and starts nothing
more on the GPU.  Per case: a random binary tree of 2 x piece + 37 nodes (piece: the ids per piece of the entry's first pass at
that k), two columns with their own parameters and masks (one-hot tips, some missing, some with two states).
  F81 family   k = 2, 4, 5, 16, 17, 64, 65, 256, 257: every lane shape <G, R>, both variants of the jump product, pieces of 1024,
               512, 256 and 2048 ids; k = 65 on 4096 + 19 tips for the pieces of 4096
  eigen models k = 2, 4, 5, 16, 17, 33, 64, 65, 128: every CR, both variants of the changes of basis, one and two bands of d
  whole tree   times, jumps, branch_jumps
  per interval times, jumps, lineages at M = 1 and at M = 7 with the first bin empty; node times are root distances
  numbering    k = 16 of each family once more in the caller's numbering (NO_HEIGHT_ORDER)
This is a record, not a test: the bits belong to one compiler and one device.
"""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TIME_LIMIT = 600   # seconds for the child (it takes well under a minute)
F81_KS = (2, 4, 5, 16, 17, 64, 65, 256, 257)
EIGEN_KS = (2, 4, 5, 16, 17, 33, 64, 65, 128)
NUMBERING_K = 16


def masks(flat, k, seed):
    rng = np.random.default_rng(100 + seed)
    out = np.ones((flat.n_nodes, k), dtype=np.int8)
    tips = flat.tips
    out[tips] = 0
    out[tips, rng.integers(0, k, size=len(tips))] = 1
    out[tips[::9]] = 1
    for t in tips[4::11]:
        out[t, rng.integers(0, k)] = 1
    return out


def models(family, k):
    from oracle import pastml_oracle as orc
    from pastml_amd import hip
    rng = np.random.default_rng(1000 + k)
    out = []
    for c in range(2):
        pi = rng.dirichlet(np.ones(k) * 2)
        rates = (0.7 + 0.4 * c, 0.01 * c, 1.0 - 0.05 * c)   # (sf, tau, tau factor)
        if family == 'f81':
            out.append((dict(kind=hip.KIND_F81, pi=pi), rates))
        else:
            R = np.triu(rng.uniform(0.05, 3, size=(k, k)), 1)
            d, a, ainv = orc.diagonalise(pi, R + R.T)
            out.append((dict(kind=hip.KIND_EIGEN, pi=pi, d=d, A=a, Ainv=ainv), rates))
    return out


def case(family, k, n_tips, tune=None, label=''):
    from pastml_amd import hip
    from pastml_amd.tree import FlatForest, annotate_dates
    flat = FlatForest.random(n_tips, seed=21, max_arity=2, zero_frac=0.0, n_trees=1)
    t = annotate_dates(flat)
    edges = np.linspace(t.min(), t.max(), 7)
    bounds = {1: np.array([t.min(), t.max()]), 7: np.concatenate([[t.min() - (edges[1] - edges[0])], edges])}
    name = '{} k={} nodes={}{}'.format(family, k, flat.n_nodes, label)
    with hip.Engine(flat, 2, k, tune=tune) as eng:
        eng.set_models(models(family, k))
        eng.set_masks(np.asarray([masks(flat, k, 3), masks(flat, k, 4)]))
        eng.marginal_pass(posterior=False, lh=False)
        whole = eng.expected_history if family == 'f81' else eng.expected_history_eigen
        through = eng.history_through_time if family == 'f81' else eng.history_through_time_eigen
        results = [('whole', ('times', 'jumps', 'branch_jumps'), whole(jumps=True, branch_jumps=True))]
        for M in (1, 7):
            results.append(('M={}'.format(M), ('times', 'jumps', 'lineages'), through(t, bounds[M])))
    for entry, names, arrays in results:
        for array_name, x in zip(names, arrays):
            x = np.ascontiguousarray(x, dtype=np.float64)
            if not np.isfinite(x).all():
                raise SystemExit('{} {} {}: not finite'.format(name, entry, array_name))
            print('{} {} {} {} sha256={}'.format(name, entry, array_name, 'x'.join(str(n) for n in x.shape),
                                                 hashlib.sha256(x.tobytes()).hexdigest()), flush=True)


def child():
    piece = lambda k: 1024 if k <= 4 else (512 if k <= 64 else 256)
    for k in F81_KS:
        case('f81', k, piece(k) + 19)
    case('f81', 65, 4096 + 19)
    case('f81', NUMBERING_K, piece(NUMBERING_K) + 19, tune={'NO_HEIGHT_ORDER': 1}, label=" caller's numbering")
    for k in EIGEN_KS:
        case('eigen', k, 512 + 19)
    case('eigen', NUMBERING_K, 512 + 19, tune={'NO_HEIGHT_ORDER': 1}, label=" caller's numbering")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', type=str, default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()
    run = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], cwd=REPO, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=TIME_LIMIT)
    sys.stdout.write(run.stdout)
    if run.returncode != 0:
        # failed, killed, aborted or hung (subprocess.run raises at the time limit): nothing more is started on the GPU after that
        raise SystemExit('the child ended with status {}: stopping here'.format(run.returncode))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(run.stdout)


if __name__ == '__main__':
    main()
