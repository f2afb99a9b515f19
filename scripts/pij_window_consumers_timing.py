"""Times the entries that read P(t) of a wide eigen model outside the sweeps, with the whole-tree batch and with windows.

Shape: scripts/pij_window_timing.py's (bench.py's eigen_k128 model: CUSTOM_RATES-shaped, k = 128, 4 characters, seeded as
there) on a balanced tree of 2^levels tips (default 16: 65 536 tips, 131 071 nodes -- the batch is 68.7 GB).  After one marginal
pass per engine, four workloads, each one call of the C-ABI as a front end makes it:
  expected   pml_expected_counts over the 4 columns;
  scenarios  pml_sample_scenarios, --repetitions (1 024) repetitions of column 0;
  simulate   pml_simulate_states, the same;
  marginal   pml_marginal_counts, --count-repetitions (1 000) repetitions of column 0.
Configurations: materialised (window 0) and one per --windows entry (branches).  A materialised call reads the batch that the
first call built (the parameters do not change); a windowed call builds every matrix it reads, run by run -- that is the price
this script measures, against 68.7 GB that need not be held.
Method: every configuration is warmed up, then `--rounds` rounds alternate over the configurations; a round times `--reps`
calls with the host clock (every call ends in its own synchronisation: it copies its result out).  Reported per configuration:
the median over the rounds and their min - max, and the memory the context holds.  The script stops if any windowed result
differs from the materialised one in any element.
--materialised-only: only window 0 -- for a checkout without the windowed entries (the parent commit's tree with its own
library; copy this script into its scripts/).  Two commits cannot share a process, so their rows come from separate runs:
alternate the runs (parent, this, parent, this) and read the difference between the repeats of ONE commit as the between-process
spread that a difference between the commits has to beat.
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
    ap.add_argument('--windows', type=int, nargs='*', default=[512, 4096, 16384])
    ap.add_argument('--repetitions', type=int, default=1024)
    ap.add_argument('--count-repetitions', type=int, default=1000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=1)
    ap.add_argument('--workloads', nargs='*', default=['expected', 'scenarios', 'simulate', 'marginal'])
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

    calls = dict(expected=lambda eng: (eng.expected_counts(0, C),),
                 scenarios=lambda eng: eng.sample_scenarios(args.repetitions, 1234567, col=0),
                 simulate=lambda eng: (eng.simulate_states(args.repetitions, 7654321, col=0),),
                 marginal=lambda eng: (eng.marginal_counts(args.count_repetitions, 2468, col=0),))
    engines = []
    try:
        for w in windows:
            eng = hip.Engine(flat, C, k, device=args.device)
            eng.set_tip_states(tips)
            eng.set_models(specs)
            if w:
                eng.pij_window_set(w)
            eng.marginal_pass(posterior=False, lh=False)
            eng.sync()
            engines.append(eng)
        for workload in args.workloads:
            call = calls[workload]
            first = []
            for eng in engines:   # warm-up: first launches, the LDS attributes, the batch of the materialised engine
                call(eng)
                first.append([np.asarray(x) for x in call(eng)])
            for w, got in zip(windows, first):
                for x, y in zip(got, first[0]):
                    if x.shape != y.shape or not np.array_equal(x, y):
                        raise SystemExit('{}: window {} differs from the materialised result'.format(workload, w))
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
            info = [eng.pij_window_info() if hasattr(eng._lib, 'pml_pij_window_info') else None for eng in engines]
            rows = []
            for i, w in enumerate(windows):
                rows.append(dict(window=w, ms_median=float(np.median(ms[i])), ms_min=float(min(ms[i])), ms_max=float(max(ms[i])),
                                 held_gb=held[i] / 1e9, window_bytes=None if info[i] is None else info[i][1],
                                 batch_bytes=None if info[i] is None else info[i][2]))
                print('{:6s} {:9s} window {:>7} : {:10.3f} ms  (min {:10.3f}  max {:10.3f})  held {:7.2f} GB'.format(
                    args.label, workload, w if w else 'batch', rows[-1]['ms_median'], rows[-1]['ms_min'], rows[-1]['ms_max'],
                    rows[-1]['held_gb']), flush=True)
            record = dict(label=args.label, workload=workload, k=k, cols=C, tips=int(flat.n_tips), nodes=int(flat.n_nodes),
                          rounds=args.rounds, reps=args.reps, repetitions=args.repetitions,
                          count_repetitions=args.count_repetitions, rows=rows, digest=hip.build_digest())
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(json.dumps(record) + '\n')
    finally:
        for eng in engines:
            eng.close()


if __name__ == '__main__':
    main()
