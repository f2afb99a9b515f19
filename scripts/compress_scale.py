#!/usr/bin/env python3
"""
The vertical collapse at scale (pastml_amd.visualisation.tree_compressor): device call, host remainder, numpy path.

    python3 scripts/compress_scale.py [--levels 18] [--cols 32] [--k 64] [--reps 5] [--out FILE]

Forests: a balanced and a ragged tree of 2^levels tips.  Inputs per forest: "walk" -- per column a slow random walk of the
state down the tree (many vertices of many sizes) -- and "one" -- every node in one state (one vertex: every count lands on
one counter).  Per (forest, input), after a warm-up call, the median of --reps calls of

  call ms     Engine.compress_vertical end to end on a context that holds the tree: upload of the sets through pageable memory,
              the kernels, download of four int32 arrays
  merged / jump / counts ms   HIP-event times of the call's three passes (no transfers), counts with the wave-level
              combining of the atomics; "plain": the counts pass with one atomic per node (same call, COMPRESS_PLAIN_ATOMICS)
  GB/s        the byte model of the merged pass over its time: per node with a parent 2 * 8 * cols * W bytes of sets + 4 (parent
              id) + per node 1 (the flag is read back by the next pass; written only where a node differs)
  host ms     compaction to vertices, child order, tip lists (tree_compressor.compact); "pajek ms": the text of the file
  numpy ms    tree_compressor.collapse_host on the same arrays (the device=False path)

It needs a GPU: without one it fails.
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


def walk_sets(flat, n_cols, k, seed, p_change):
    rng = np.random.default_rng(seed)
    N = flat.n_nodes
    state = rng.integers(k, size=(n_cols, N))
    change = rng.random((n_cols, N)) < p_change
    for lvl in range(1, flat.n_td_levels):
        a, b = flat.td_offsets[lvl], flat.td_offsets[lvl + 1]
        state[:, a:b] = np.where(change[:, a:b], state[:, a:b], state[:, flat.parent[a:b]])
    return one_hot_words(state, k)


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def merged_bytes(flat, n_cols, W):
    with_parent = int((flat.parent >= 0).sum())
    return with_parent * (2 * 8 * n_cols * W + 4) + flat.n_nodes


def measure(label, flat, sets, reps, lines):
    n_cols, N, W = sets.shape
    out = {}
    for tune in (None, dict(COMPRESS_PLAIN_ATOMICS=1)):
        with hip.Engine.tree_only(flat, tune=tune) as eng:
            eng.profile_enable()                   # (the event brackets of compress_vertical_info)
            result = eng.compress_vertical(sets)   # warm-up: code objects, first allocations
            infos = []

            def call():
                eng.compress_vertical(sets)
                infos.append(eng.compress_vertical_info())

            call_ms = median_ms(call, reps)
            passes = np.median(np.array([i[:3] for i in infos]), axis=0)
            out['plain' if tune else 'combined'] = (call_ms, passes, infos[0][3], result)
    for a, b in zip(out['combined'][3], out['plain'][3]):
        assert np.array_equal(a, b)
    call_ms, passes, rounds, result = out['combined']
    host = tc.collapse_host(flat, sets)
    for a, b in zip(result, host):
        assert np.array_equal(a, b)
    numpy_ms = median_ms(lambda: tc.collapse_host(flat, sets), max(1, reps // 2))
    host_ms = median_ms(lambda: tc.compact(flat, *result), reps)

    compressed = tc.compact(flat, *result, columns=['c{:02d}'.format(i) for i in range(n_cols)],
                            states=[np.array(['s{:03d}'.format(j) for j in range(64 * W)])] * n_cols, words=list(sets))
    pajek_ms = median_ms(lambda: tc.pajek_lines(compressed), 1)
    gbs = merged_bytes(flat, n_cols, W) / (passes[0] * 1e-3) / 1e9
    lines.append('{:>22} {:8d} {:5d} {:9d} {:7d} {:9.2f} {:9.3f} {:8.3f} {:9.3f} {:9.3f} {:8.1f} {:9.1f} {:9.1f} {:9.1f}'.format(
        label, N, flat.n_td_levels, len(compressed.top), rounds, call_ms, passes[0], passes[1], passes[2], out['plain'][1][2],
        gbs, host_ms, pajek_ms, numpy_ms))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--levels', type=int, default=18)
    ap.add_argument('--cols', type=int, default=32)
    ap.add_argument('--k', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if hip.device_count() < 1:
        raise SystemExit('compress_scale.py needs a GPU')
    n_tips = 1 << args.levels
    W = (args.k + 63) // 64
    lines = ['vertical collapse: 2^{} tips x {} columns x k = {} (W = {}); medians of {} calls after a warm-up call'.format(
        args.levels, args.cols, args.k, W, args.reps),
        '{:>22} {:>8} {:>5} {:>9} {:>7} {:>9} {:>9} {:>8} {:>9} {:>9} {:>8} {:>9} {:>9} {:>9}'.format(
            'forest / input', 'nodes', 'depth', 'vertices', 'rounds', 'call ms', 'merged ms', 'jump ms', 'counts ms', 'plain ms',
            'GB/s', 'host ms', 'pajek ms', 'numpy ms')]
    print('\n'.join(lines), flush=True)
    for name, flat in (('balanced', FlatForest.balanced(args.levels)),
                       ('ragged', FlatForest.random(n_tips, seed=1, max_arity=3))):
        flat.nodes = None
        walk = walk_sets(flat, args.cols, args.k, seed=2, p_change=0.02 / args.cols)
        measure(name + ' / walk', flat, walk, args.reps, lines)
        one = np.ones_like(walk)
        measure(name + ' / one', flat, one, args.reps, lines)
    lines.append('merged-pass byte model: (nodes - roots) * (2 * 8 * cols * W + 4) + nodes bytes')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
