#!/usr/bin/env python3
"""
Performance record of the forward simulator (pml_simulate_states).  Three modes:

    simulate_scale.py [--iters N]                       each case: 2 warm-up calls, then N timed calls (HIP events around
                                                        Engine.simulate_states, which includes the copy of the [N, n_rep]
                                                        states to the host); one JSON line per case
    simulate_scale.py --trace kernel_trace.csv          device time of the simulator's kernels per call, from a
                                                        `rocprofv3 --kernel-trace --output-format csv` run of the first
                                                        mode (same --iters / --cases), against the two models below
    simulate_scale.py --pmc counter_collection.csv ...  SQ counters of the subtree-walk launch of the first case, from
                                                        `rocprofv3 --pmc ...` runs of their own
scripts/simulate_profile.sh runs all three.

Models:
    bytes:        2 B per draw at uint8 (the parent's state read, the child's written), 4 B at uint16; at 6 TB/s
    instructions: per wavefront step (64 lanes x 4 draws of one node) one Philox-4x32-10 call and 4 bisections, ~1150
                  SIMD cycles (see VALU_CYCLES_PER_WAVE_STEP)
"""
import argparse
import collections
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pastml_amd import hip  # noqa: E402
from pastml_amd.annotation import ForestStats  # noqa: E402
from pastml_amd.models._closed_form import F81Model  # noqa: E402
from pastml_amd.models._eigen import JTTModel  # noqa: E402
from pastml_amd.tree import FlatForest  # noqa: E402

HBM_BYTES_PER_S = 6.0e12
# VALU issue of one wavefront step (64 lanes x 4 draws of one node): a wave64 VALU instruction issues over 4 cycles, a
# quarter-rate one over 16.  Philox-4x32-10: 20 v_mad_u64_u32 (quarter rate) + ~60 full-rate xor / add / move ~ 560 cycles;
# the 4 draws: u and its scaling in FP64, then a bisection of log2(k) steps (LDS read, FP64 compare, two selects) each
# ~ 590 cycles at k = 64 -- ~1150 cycles per step; 256 CUs x 4 SIMDs x 2.4 GHz
VALU_CYCLES_PER_WAVE_STEP = 1150.0
SIMD_CYCLES_PER_S = 256 * 4 * 2.4e9


def caterpillar(depth, seed=5):
    n = 2 * depth + 1
    parent = np.full(n, -1, dtype=np.int32)
    n_children = np.zeros(n, dtype=np.int32)
    first_child = np.zeros(n, dtype=np.int32)
    spine = [0] + [2 * d - 1 for d in range(1, depth + 1)]
    for d in range(depth):
        p = spine[d]
        n_children[p] = 2
        first_child[p] = 2 * d + 1
        parent[2 * d + 1] = p
        parent[2 * d + 2] = p
    dist = np.random.default_rng(seed).uniform(0.001, 0.2, size=n)
    return FlatForest(parent, n_children, first_child, dist, np.array([0]))


def model_for(name, k, flat):
    roots = flat.to_tree_nodes() if flat.nodes is None else [flat.nodes[r] for r in flat.roots]
    fs = ForestStats(roots)
    if name == 'F81':
        pi = np.random.default_rng(k).dirichlet(np.ones(k) * 2)
        return F81Model(states=np.array(['s{}'.format(i) for i in range(k)]), forest_stats=fs, sf=1.0, frequencies=pi)
    return JTTModel(forest_stats=fs, sf=1.0)




CASES = collections.OrderedDict([
    # name: (model, k, n_rep, nodes, forest)
    ('balanced20_f81_k64', ('F81', 64, 1000, 2 ** 21 - 1, lambda: FlatForest.balanced(20))),
    ('balanced18_jtt', ('JTT', 20, 1000, 2 ** 19 - 1, lambda: FlatForest.balanced(18))),
    ('caterpillar_1e4', ('F81', 4, 1000, 2 * 10000 + 1, lambda: caterpillar(10000))),
])
WARMUP = 2
WALK_NODES_CASE1 = 2 ** 21 - 1 - (2 ** 11 - 1)   # nodes of the first case's subtree walk (below the frontier depth 11)


def models(name):
    """(draws, state bytes, bytes-model ms, instruction-model ms) of a case"""
    mname, k, n_rep, nodes, _ = CASES[name]
    draws = float(nodes) * n_rep
    nbytes = 2.0 * (1 if k <= 256 else 2) * draws
    return draws, nbytes, 1e3 * nbytes / HBM_BYTES_PER_S, 1e3 * (draws / 256.0) * VALU_CYCLES_PER_WAVE_STEP / SIMD_CYCLES_PER_S


def run(name, iters):
    mname, k, n_rep, nodes, make = CASES[name]
    flat = make()
    model = model_for(mname, k, flat)
    with hip.Engine(flat, 1, k) as eng:
        eng.set_models([model])
        for _ in range(WARMUP):
            eng.simulate_states(n_rep, 1)
        ms = []
        for i in range(iters):
            eng.timer_start()
            eng.simulate_states(n_rep, 100 + i)
            ms.append(eng.timer_stop())
    draws, nbytes, _, _ = models(name)
    print(json.dumps(dict(case=name, model=mname, k=k, nodes=nodes, n_rep=n_rep,
                          ms_per_call_with_copy=round(float(np.median(ms)), 3),
                          state_bytes=float('{:.3g}'.format(nbytes)), draws=float('{:.3g}'.format(draws)))), flush=True)


def summarize_trace(path, names, iters):
    """Calls are runs of simulate_kernel launches (each call starts with the per-branch preparation kernel)."""
    calls, cur = [], []
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp'])):
        if 'simulate_kernel' not in r['Kernel_Name']:
            if cur:
                calls.append(cur)
                cur = []
            continue
        cur.append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6)
    if cur:
        calls.append(cur)
    per = WARMUP + iters
    if len(calls) != per * len(names):
        raise SystemExit('{} calls traced, {} expected'.format(len(calls), per * len(names)))
    for j, name in enumerate(names):
        timed = calls[j * per + WARMUP:(j + 1) * per]
        dev = float(np.median([sum(c) for c in timed]))
        walk = float(np.median([max(c) for c in timed]))
        draws, nbytes, hbm_ms, valu_ms = models(name)
        print(json.dumps(dict(case=name, launches=len(timed[0]), device_ms=round(dev, 3), walk_launch_ms=round(walk, 3),
                              draws_per_s=float('{:.3g}'.format(draws / (dev * 1e-3))),
                              state_tb_per_s=round(nbytes / (dev * 1e-3) / 1e12, 3),
                              hbm_model_ms=round(hbm_ms, 3), hbm_fraction=round(hbm_ms / dev, 3),
                              valu_model_ms=round(valu_ms, 3), valu_fraction=round(valu_ms / dev, 3))), flush=True)


def summarize_pmc(paths):
    """SQ counters of the largest simulate_kernel dispatches (the subtree walk of the first case), averaged over them."""
    acc = collections.defaultdict(list)
    for path in paths:
        disp = collections.defaultdict(dict)
        for r in csv.DictReader(open(path)):
            if 'simulate_kernel' not in r['Kernel_Name']:
                continue
            d = disp[int(r['Dispatch_Id'])]
            d['grid'] = int(r['Grid_Size'])
            d[r['Counter_Name']] = d.get(r['Counter_Name'], 0.0) + float(r['Counter_Value'])
        big = max(d['grid'] for d in disp.values())
        for d in disp.values():
            if d['grid'] == big:
                for name, v in d.items():
                    if name != 'grid':
                        acc[name].append(v)
    c = {name: float(np.mean(v)) for name, v in acc.items()}
    print(json.dumps({name: float('{:.4g}'.format(v)) for name, v in sorted(c.items())}))
    simds = 256 * 4
    out = {}
    if 'GRBM_GUI_ACTIVE' in c:
        cycles = c['GRBM_GUI_ACTIVE'] / 8.0   # (rocprofv3 sums it over the 8 XCDs)
        out['kernel_cycles'] = cycles
        # SQ_WAVE_CYCLES / SQ_ACTIVE_INST_* / SQ_WAIT_* count quad-cycles, summed over the waves
        if 'SQ_WAVE_CYCLES' in c:
            out['mean_resident_waves_per_simd'] = 4.0 * c['SQ_WAVE_CYCLES'] / (simds * cycles)
        if 'SQ_ACTIVE_INST_VALU' in c:
            out['valu_issue_fraction_per_simd'] = 4.0 * c['SQ_ACTIVE_INST_VALU'] / (simds * cycles)
        if 'SQ_ACTIVE_INST_ANY' in c:
            out['any_issue_fraction_per_simd'] = 4.0 * c['SQ_ACTIVE_INST_ANY'] / (simds * cycles)
    if 'SQ_WAIT_ANY' in c and 'SQ_WAVE_CYCLES' in c:
        out['wave_cycles_waiting_fraction'] = c['SQ_WAIT_ANY'] / c['SQ_WAVE_CYCLES']
    steps = WALK_NODES_CASE1 * 1000 / 256.0   # wavefront steps of the walk (4 repetitions x 64 lanes each)
    for name in ('SQ_INSTS_VALU', 'SQ_INSTS_SALU', 'SQ_INSTS_LDS', 'SQ_INSTS_VMEM_RD', 'SQ_INSTS_VMEM_WR'):
        if name in c:
            out[name.lower() + '_per_wave_step'] = c[name] / steps
    print(json.dumps({name: float('{:.4g}'.format(v)) for name, v in out.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--trace', help='kernel_trace.csv of a rocprofv3 run of this script (same --iters / --cases)')
    ap.add_argument('--pmc', nargs='+', help='counter_collection.csv files of rocprofv3 --pmc runs of the first case')
    a = ap.parse_args()
    names = a.cases.split(',')
    for name in names:
        if name not in CASES:
            raise SystemExit('unknown case ' + name)
    if a.trace:
        summarize_trace(a.trace, names, a.iters)
    elif a.pmc:
        summarize_pmc(a.pmc)
    else:
        for name in names:
            run(name, a.iters)


if __name__ == '__main__':
    main()
