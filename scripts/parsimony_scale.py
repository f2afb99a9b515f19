#!/usr/bin/env python3
"""
Host path against device path of the parsimonious methods (MP = ACCTRAN + DOWNPASS + DELTRAN) over forest sizes:

    python scripts/parsimony_scale.py [--path host|device|both] [--sizes name,name,...] [--out FILE]

Per size one child process per path, each under its own time limit; the run stops at the first child that fails.  Both
paths get the same forest (FlatForest.random, seeded) and the same annotation (one state per tip, 10 % of the tips none),
and do everything parsimonious_acr does: packing of the annotation, the passes, node features, result dictionaries.

  host     pastml_amd.parsimony.parsimonious_acr per character (the only path before the device one existed).  On the
           large sizes --host-chars characters are timed and the figure is scaled to all of them (the path is a loop over
           the characters); the table says how many were timed.
  device   pastml_amd.parsimony.parsimonious_acr_batch: a fresh tree-only context, tree upload, one pml_parsimony call,
           features.  Timed on the second call of the process (the first pays for loading the library and the runtime);
           `passes` is the HIP-event time of the kernels of that call, `launches` its kernel launches.

The crossover for PASTML_AMD_PARSIMONY=auto is the smallest work = nodes x characters x words per set from which the
device is faster; pastml_amd.parsimony.AUTO_MIN_WORK is that, rounded up to a power of two.
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

# name: (tips, largest number of children, characters, states)
SIZES = {
    't152x1': (152, 2, 1, 4), 't152x8': (152, 2, 8, 4), 't500x1': (500, 2, 1, 4), 't1000x1': (1000, 2, 1, 4),
    't2000x1': (2000, 2, 1, 4), 't4000x1': (4000, 2, 1, 4), 't8000x1': (8000, 2, 1, 4), 't16000x1': (16000, 2, 1, 4),
    't3619x91k64': (3619, 4, 91, 64), 't100000x16k20': (100000, 3, 16, 20),
    't262144x32k4': (262144, 2, 32, 4), 't262144x32k64': (262144, 2, 32, 64),
}


def one(name, path, host_chars):
    import numpy as np
    from pastml_amd import hip, parsimony as P
    from pastml_amd.tree import AnnotationColumn
    from pastml_amd.tree import FlatForest, get_flat_forest
    tips, arity, m, k = SIZES[name]
    roots = [n for n in FlatForest.random(tips, seed=tips % 1000 + arity, max_arity=arity).nodes if n.up is None]
    flat = get_flat_forest(roots)
    rng = np.random.default_rng(k + m)
    states = np.array(['s{:03d}'.format(i) for i in range(k)])
    is_tip = np.asarray(flat.n_children) == 0
    names = ['c{}'.format(j) for j in range(m)]
    for c in names:
        codes = np.where(is_tip & (rng.random(flat.n_nodes) >= 0.1), rng.integers(k, size=flat.n_nodes), -2).astype(np.int64)
        flat.set_column(c, AnnotationColumn(codes, states, {}))
    out = dict(name=name, path=path, nodes=flat.n_nodes, tips=flat.n_tips, chars=m, k=k,
               work=flat.n_nodes * m * ((k + 63) // 64))
    if path == 'host':
        timed = m if flat.n_nodes * m * k <= 5e7 else min(m, host_chars)
        if flat.n_nodes < 50000:
            P.parsimonious_acr(roots, names[0], P.MP, states, flat.n_nodes, flat.n_tips)   # (imports, caches of the forest)
        t0 = time.perf_counter()
        res = [P.parsimonious_acr(roots, c, P.MP, states, flat.n_nodes, flat.n_tips) for c in names[:timed]]
        out.update(seconds=(time.perf_counter() - t0) * m / timed, timed_chars=timed)
    else:
        info = []
        real = hip.Engine.parsimony

        def noted(self, *a):
            r = real(self, *a)
            info.append(self.parsimony_info())
            return r

        hip.Engine.parsimony = noted
        P.parsimonious_acr_batch(roots, names[:1], [P.MP], [states], flat.n_nodes, flat.n_tips)   # (library, runtime)
        t0 = time.perf_counter()
        res = P.parsimonious_acr_batch(roots, names, [P.MP] * m, [states] * m, flat.n_nodes, flat.n_tips)
        out.update(seconds=time.perf_counter() - t0, launches=info[-1][0], passes_ms=info[-1][1])
    out['steps'] = [int(r[P.STEPS]) for r in res[0]]
    print('RESULT ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--path', default='both', choices=['host', 'device', 'both'])
    ap.add_argument('--sizes', default=','.join(SIZES))
    ap.add_argument('--host-chars', type=int, default=2)
    ap.add_argument('--limit', type=int, default=300, help='seconds per child process')
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.path, args.host_chars)
    lines = ['{:>16} {:>8} {:>5} {:>4} {:>10} {:>11} {:>11} {:>9} {:>9} {:>7}'.format(
        'size', 'nodes', 'chars', 'k', 'work', 'host s', 'device s', 'passes ms', 'launches', 'ratio')]
    print(lines[0], flush=True)
    for name in args.sizes.split(','):
        got = {}
        for path in (['host', 'device'] if args.path == 'both' else [args.path]):
            cmd = [sys.executable, os.path.abspath(__file__), '--one', name, '--path', path, '--host-chars', str(args.host_chars)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=args.limit, universal_newlines=True)
            except subprocess.TimeoutExpired:
                print('{} {}: no answer within {} s; stopping'.format(name, path, args.limit), flush=True)
                return 1
            if p.returncode != 0:
                print(p.stdout[-2000:])
                print('{} {}: exit status {}; stopping'.format(name, path, p.returncode), flush=True)
                return 1
            got[path] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
        if len(got) == 2 and got['host']['steps'] != got['device']['steps']:
            print('{}: the two paths disagree: {} / {}'.format(name, got['host']['steps'], got['device']['steps']))
            return 1
        any_ = next(iter(got.values()))
        h, d = got.get('host'), got.get('device')
        host_s = '{:.4f}{}'.format(h['seconds'], '' if h['timed_chars'] == h['chars'] else '*{}'.format(h['timed_chars'])) if h else '-'
        line = '{:>16} {:>8} {:>5} {:>4} {:>10} {:>11} {:>11} {:>9} {:>9} {:>7}'.format(
            name, any_['nodes'], any_['chars'], any_['k'], any_['work'], host_s,
            '{:.4f}'.format(d['seconds']) if d else '-', '{:.3f}'.format(d['passes_ms']) if d else '-',
            d['launches'] if d else '-', '{:.1f}'.format(h['seconds'] / d['seconds']) if h and d else '-')
        lines.append(line)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
