#!/usr/bin/env python3
"""
The trimming at scale (pastml_amd.visualisation.tree_compressor): the device call per phase against ``trim_host``.

    python3 scripts/compress_trim_scale.py [--tips 262144] [--cols 4] [--k 4] [--p_change 0.05] [--threshold 15] [--reps 3]
                                           [--out FILE]

A random tree, per column a slow random walk of one state down it; the vertical collapse and the horizontal merging on the
host, then ``Engine.compress_trim`` on the live vertices (the events of ``compress_trim_info`` per phase, and the call end to
end with its transfers, host checks and the selection of the threshold) and ``trim_host`` on the same arrays.  Prints the
vertices before and after, the threshold, levels, rounds, launches and the medians of the times.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pastml_amd import hip  # noqa: E402
from pastml_amd.tree import FlatForest  # noqa: E402
from pastml_amd.visualisation import tree_compressor as tc  # noqa: E402
from compress_horizontal_scale import walk_words  # noqa: E402


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--tips', type=int, default=262144)
    parser.add_argument('--cols', type=int, default=4)
    parser.add_argument('--k', type=int, default=4)
    parser.add_argument('--p_change', type=float, default=0.05)
    parser.add_argument('--threshold', type=int, default=tc.REASONABLE_NUMBER_OF_TIPS)
    parser.add_argument('--reps', type=int, default=3)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    if hip.device_count() < 1:
        raise SystemExit('compress_trim_scale.py needs a GPU')
    flat = FlatForest.random(args.tips, seed=1, max_arity=3)
    sets = walk_words(flat, args.cols, args.k, 2, args.p_change)
    compressed = tc.compact(flat, *tc.collapse_host(flat, sets), columns=['c{:02d}'.format(i) for i in range(args.cols)],
                            states=[np.arange(args.k)] * args.cols, words=list(sets))
    merged = tc.collapse_horizontally(compressed, tip_size_threshold=args.threshold, device=False)
    L = merged.n_vertices
    has_child = np.zeros(L, dtype=bool)
    has_child[merged.parent[merged.parent >= 0]] = True
    tree = compressed.tree[merged.vertex]
    gate = np.bincount(tree[~has_child], minlength=len(merged.second_pass)) > args.threshold
    arrays = (merged.parent.astype(np.int32), tree.astype(np.int32), merged.n_tips_total.astype(np.int32),
              merged.width.astype(np.int32), tc.stacked_sets([w[merged.vertex] for w in compressed.words], L), args.threshold, gate)
    call_ms, infos = [], []
    with hip.Engine.tree_only(flat) as eng:
        eng.profile_enable()
        eng.compress_trim(*arrays)   # warm-up: code objects, first allocations
        for _ in range(args.reps):
            t0 = time.perf_counter()
            device = eng.compress_trim(*arrays)
            call_ms.append(1e3 * (time.perf_counter() - t0))
            infos.append(eng.compress_trim_info())
    host_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        host = tc.trim_host(*arrays)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    for d, h in zip(device, host):
        assert d.dtype == h.dtype and np.array_equal(d, h, equal_nan=d.dtype == np.float64)
    tsize, keep, spliced, new_parent, moved, threshold = device
    info = infos[-1]
    phases = np.median([i['ms'] for i in infos], axis=0)
    lines = ['tips {}  cols {}  k {}  p_change {}  tip_size_threshold {}'.format(args.tips, args.cols, args.k, args.p_change, args.threshold),
             'live vertices {}  kept {}  mediators {}  moved {}  threshold {}'.format(L, int(keep.sum()), int(spliced.sum()),
                                                                                     int(moved.sum()), threshold.tolist()),
             'levels {}  rounds {}  launches {}  scan tile {}'.format(info['levels'], info['rounds'], info['launches'], info['scan_tile']),
             'events ms (sizes, removal, mediators)  {}'.format(', '.join('{:.3f}'.format(x) for x in phases)),
             'device call end to end (transfers, host checks, threshold)  {:.2f} ms   kernels by events {:.3f} ms'.format(
                 np.median(call_ms), float(phases.sum())),
             'trim_host (numpy)  {:.2f} ms'.format(np.median(host_ms))]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
