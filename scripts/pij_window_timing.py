"""Times the sweeps that read P(t) of a wide eigen model with the whole-tree batch and with windows of several sizes.

Shape: bench.py's eigen_k128 model (CUSTOM_RATES-shaped, k = 128, 4 characters, seeded as there) on a balanced tree of
2^levels tips (default 16: 65 536 tips, 131 071 nodes -- the batch is 68.7 GB).  Two workloads, each a call as an optimiser or a
reconstruction makes it (model upload included, so P(t) is new every time):
  joint     the joint sweep, pml_bottom_up(is_marginal = 0) -- reads P(t) under the default switches;
  marginal  pml_marginal_pass with the fused sum sweeps switched off (NO_EIGEN_GEMM) -- both sweeps read P(t).
Configurations: materialised (window 0) and one per --windows entry (branches).  With 4 characters and k = 128 a branch of the
window is 512 KiB, so 128 branches lie well inside the 256 MiB last-level cache, 512 fill it, 4 096 are eight times larger.
Method: every configuration is warmed up (its captured sweeps are replayed afterwards), then `--rounds` rounds alternate over
the configurations; a round times `--reps` calls behind one synchronisation with the host clock.  Reported per configuration:
the median over the rounds and their min - max, the spread a difference has to beat.  ln L of every windowed configuration
must equal the materialised one's bit for bit.
--materialised-only: only window 0 -- for a checkout without the window (the parent commit's tree with its own library; copy this
script into its scripts/).  Two commits cannot share a process, so their rows come from separate runs: alternate the runs
(parent, this, parent, this) and read the difference between the repeats of ONE commit as the between-process spread that a
difference between the commits has to beat.
Writes one JSON line per workload to --out (appending), with --label in it, and prints a table."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--levels', type=int, default=16)
    ap.add_argument('--k', type=int, default=128)
    ap.add_argument('--cols', type=int, default=4)
    ap.add_argument('--windows', type=int, nargs='*', default=[128, 512, 4096])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--label', default='this')
    ap.add_argument('--materialised-only', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--device', type=int, default=0)
    args = ap.parse_args()

    from pastml_amd import hip, synthetic
    from pastml_amd.models._eigen import get_diagonalisation
    k, C = args.k, args.cols
    flat = synthetic.balanced_forest(args.levels)
    rng = np.random.default_rng(k)
    rates = np.triu(rng.uniform(0.05, 3.0, size=(k, k)), 1)
    rates = rates + rates.T
    specs = []
    for c in range(C):
        pi = rng.dirichlet(np.ones(k) * 4)
        d, a, ainv = get_diagonalisation(pi, rates)
        specs.append((dict(kind=2, pi=pi, d=d, A=a, Ainv=ainv), (1.0, 0.0, 1.0)))
    tips = np.stack([synthetic.tip_states(flat.n_tips, k, c) for c in range(C)])
    windows = [0] + ([] if args.materialised_only else [min(w, flat.n_nodes) for w in args.windows])
    print('# {}: k = {}, {} characters, {} tips, {} nodes; library {} ({})'.format(
        args.label, k, C, flat.n_tips, flat.n_nodes, hip.library_path(), hip.build_digest()), flush=True)

    for workload, tune in (('joint', {}), ('marginal', dict(NO_EIGEN_GEMM=1))):
        engines = []
        try:
            for w in windows:
                eng = hip.Engine(flat, C, k, device=args.device, tune=tune)
                eng.set_tip_states(tips)
                eng.set_models(specs)
                if w:
                    eng.pij_window_set(w)
                engines.append(eng)

            def call(eng):
                eng.set_models(specs)
                if workload == 'joint':
                    return eng.bottom_up(False)
                return eng.marginal_pass(posterior=False, lh=False)[0]

            lnl = []
            for eng in engines:   # warm-up: first launches, the capture; the second call replays
                call(eng)
                lnl.append(call(eng))
                eng.sync()
            for w, v in zip(windows, lnl):
                if not np.array_equal(v, lnl[0]):
                    raise SystemExit('window {}: ln L {} differs from the materialised {}'.format(w, v, lnl[0]))
            ms = [[] for _ in engines]
            for _ in range(args.rounds):
                for i, eng in enumerate(engines):
                    eng.sync()
                    t0 = time.perf_counter()
                    for _r in range(args.reps):
                        call(eng)
                    eng.sync()
                    ms[i].append((time.perf_counter() - t0) / args.reps * 1e3)
            held = [eng.memory()[0] for eng in engines]
            info = [eng.pij_window_info() if hasattr(eng._lib, 'pml_pij_window_info') and not args.materialised_only else None
                    for eng in engines]
        finally:
            for eng in engines:
                eng.close()
        rows = []
        for i, w in enumerate(windows):
            rows.append(dict(window=w, ms_median=float(np.median(ms[i])), ms_min=float(min(ms[i])), ms_max=float(max(ms[i])),
                             held_gb=held[i] / 1e9, window_bytes=None if info[i] is None else info[i][1],
                             batch_bytes=None if info[i] is None else info[i][2]))
            print('{:6s} {:9s} window {:>7} : {:9.3f} ms  (min {:9.3f}  max {:9.3f})  held {:7.2f} GB'.format(
                args.label, workload, w if w else 'batch', rows[-1]['ms_median'], rows[-1]['ms_min'], rows[-1]['ms_max'],
                rows[-1]['held_gb']), flush=True)
        record = dict(label=args.label, workload=workload, k=k, cols=C, tips=int(flat.n_tips), nodes=int(flat.n_nodes),
                      rounds=args.rounds, reps=args.reps, lnl=[float(v) for v in lnl[0]], rows=rows, digest=hip.build_digest())
        if args.out:
            with open(args.out, 'a') as f:
                f.write(json.dumps(record) + '\n')


if __name__ == '__main__':
    main()
