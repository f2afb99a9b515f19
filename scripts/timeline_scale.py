#!/usr/bin/env python3
"""
The timeline at scale (pastml_amd.visualisation.timeline): the device call per stage against ``timeline_host``.

    python3 scripts/timeline_scale.py [--tips 262144] [--cols 4] [--k 4] [--p_change 0.05] [--threshold 15] [--reps 3] [--out FILE]

A random tree, per column a slow random walk of one state down it; the whole compressor on the host, then for each timeline
type with the reference's choice of milestones (M <= 9): ``Engine.timeline`` on the arrays of ``timeline_arrays`` (the events of
``timeline_info`` per stage, and the call end to end with its transfers and host checks) and ``timeline_host`` on the same
arrays.  Prints the sizes, levels, launches and the medians of the times; the results of the two paths are compared.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pastml_amd import hip  # noqa: E402
from pastml_amd.tree import FlatForest  # noqa: E402
from pastml_amd.visualisation import timeline as tl  # noqa: E402
from pastml_amd.visualisation import tree_compressor as tc  # noqa: E402
from compress_horizontal_scale import walk_words  # noqa: E402

STAGES = ('dates', 'get_date', 'bins', 'roles', 'tips below', 'vertices')


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
        raise SystemExit('timeline_scale.py needs a GPU')
    flat = FlatForest.random(args.tips, seed=1, max_arity=3)
    sets = walk_words(flat, args.cols, args.k, 2, args.p_change)
    compressed = tc.compact(flat, *tc.collapse_host(flat, sets), columns=['c{:02d}'.format(i) for i in range(args.cols)],
                            states=[np.arange(args.k)] * args.cols, words=list(sets))
    merged = tc.collapse_horizontally(compressed, tip_size_threshold=args.threshold, device=False)
    trimmed = tc.trim(merged, tip_size_threshold=args.threshold, device=False)
    t0 = time.perf_counter()
    arrays = tl.timeline_arrays(trimmed)
    arrays_ms = 1e3 * (time.perf_counter() - t0)
    lines = ['tips {}  nodes {}  cols {}  k {}  p_change {}  tip_size_threshold {}'.format(
                 args.tips, flat.n_nodes, args.cols, args.k, args.p_change, args.threshold),
             'vertices {}  configurations {}  alive nodes {}  levels {}'.format(
                 trimmed.n_vertices, len(arrays.top), int(arrays.alive.sum()), flat.n_td_levels),
             'timeline_arrays (host, both paths)  {:.1f} ms'.format(arrays_ms)]
    with hip.Engine.tree_only(flat) as eng:
        eng.profile_enable()
        for timeline_type in tl.TIMELINE_TYPES:
            milestones = tl.timeline_host(arrays, timeline_type=timeline_type)['milestones']
            tl.timeline_device(arrays, eng, timeline_type=timeline_type, milestones=milestones)   # warm-up
            call_ms, infos, host_ms = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                device = tl.timeline_device(arrays, eng, timeline_type=timeline_type, milestones=milestones)
                call_ms.append(1e3 * (time.perf_counter() - t0))
                infos.append(eng.timeline_info())
            for _ in range(args.reps):
                t0 = time.perf_counter()
                host = tl.timeline_host(arrays, timeline_type=timeline_type, milestones=milestones)
                host_ms.append(1e3 * (time.perf_counter() - t0))
            for name in ('date', 'get_date'):
                assert np.array_equal(device[name].view(np.int64), host[name].view(np.int64)), name
            for name in tl.COUNTS + ('first_milestone',):
                assert np.array_equal(device[name], host[name]), name
            stages = np.median([i['ms'] for i in infos], axis=0)
            info = infos[-1]
            lines += ['{}  M {}  launches {} (date sweep {}, fuse width {})'.format(
                          timeline_type, len(milestones), info['launches'], info['date_launches'], info['fuse_width']),
                      '  events ms  ' + '  '.join('{} {:.3f}'.format(s, x) for s, x in zip(STAGES, stages)) +
                      '  sum {:.3f}'.format(float(stages.sum())),
                      '  device call end to end (transfers, host checks)  {:.2f} ms   timeline_host (numpy)  {:.2f} ms'.format(
                          np.median(call_ms), np.median(host_ms))]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
