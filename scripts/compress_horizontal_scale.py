#!/usr/bin/env python3
"""
The horizontal merging at scale (pastml_amd.visualisation.tree_compressor): device passes against the numpy restatement.

    python3 scripts/compress_horizontal_scale.py [--tips 262144] [--cols 4] [--k 4] [--p_change 0.05] [--reps 3] [--out FILE]

A random tree, per column a slow random walk of one state down it; the vertical collapse on the host, then
``collapse_horizontally`` on the device (a context that holds the tree; the events of ``compress_horizontal_info`` per pass)
and with ``device=False``.  Prints vertices before and after, levels, launches, table slots and the medians of the times.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pastml_amd import hip  # noqa: E402
from pastml_amd.batch import one_hot_words  # noqa: E402
from pastml_amd.tree import FlatForest  # noqa: E402
from pastml_amd.visualisation import tree_compressor as tc  # noqa: E402


def walk_words(flat, n_cols, k, seed, p_change):
    rng = np.random.default_rng(seed)
    N = flat.n_nodes
    state = rng.integers(k, size=(n_cols, N))
    change = rng.random((n_cols, N)) < p_change
    for lvl in range(1, flat.n_td_levels):
        a, b = flat.td_offsets[lvl], flat.td_offsets[lvl + 1]
        state[:, a:b] = np.where(change[:, a:b], state[:, a:b], state[:, flat.parent[a:b]])
    return one_hot_words(state, k)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--tips', type=int, default=262144)
    parser.add_argument('--cols', type=int, default=4)
    parser.add_argument('--k', type=int, default=4)
    parser.add_argument('--p_change', type=float, default=0.05)
    parser.add_argument('--reps', type=int, default=3)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    if hip.device_count() < 1:
        raise SystemExit('compress_horizontal_scale.py needs a GPU')
    flat = FlatForest.random(args.tips, seed=1, max_arity=3)
    sets = walk_words(flat, args.cols, args.k, 2, args.p_change)
    compressed = tc.compact(flat, *tc.collapse_host(flat, sets), columns=['c{:02d}'.format(i) for i in range(args.cols)],
                            states=[np.arange(args.k)] * args.cols, words=list(sets))
    lines = []

    class Timed(object):
        def __init__(self, eng):
            self.eng, self.infos, self.ms = eng, [], []

        def compress_horizontal(self, *a):
            t0 = time.perf_counter()
            out = self.eng.compress_horizontal(*a)
            self.ms.append(1e3 * (time.perf_counter() - t0))
            self.infos.append(self.eng.compress_horizontal_info())
            return out

    with hip.Engine.tree_only(flat) as eng:
        eng.profile_enable()
        tc.collapse_horizontally(compressed, engine=eng)   # warm-up: code objects, first allocations
        runs = []
        for _ in range(args.reps):
            timed = Timed(eng)
            merged = tc.collapse_horizontally(compressed, engine=timed)
            runs.append(timed)
    calls = np.median([sum(r.ms) for r in runs])
    events = np.median([sum(sum(i['ms']) for i in r.infos) for r in runs])
    host_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        host = tc.collapse_horizontally(compressed, device=False)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(host.vertex, merged.vertex) and np.array_equal(host.width, merged.width)
    info = runs[-1].infos
    lines.append('tips {}  cols {}  k {}  p_change {}'.format(args.tips, args.cols, args.k, args.p_change))
    lines.append('vertices {} -> {}  groups per pass {}  passes {}'.format(compressed.n_vertices, merged.n_vertices,
                                                                           merged.merged_groups, len(info)))
    for i, one in enumerate(info):
        lines.append('pass {}: levels {}  launches {}  table slots {}  events ms (states, levels, down) {}'.format(
            i + 1, one['levels'], one['launches'], one['table_slots'], ', '.join('{:.3f}'.format(x) for x in one['ms'])))
    lines.append('device passes, calls end to end (transfers, host planning)  {:.2f} ms   kernels by events {:.2f} ms'.format(calls, events))
    lines.append('collapse_horizontally device=False (numpy, member lists included)  {:.2f} ms'.format(np.median(host_ms)))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
