"""
Measures what tests/test_gpu_optimiser_points.py asserts (profiles/optimiser_points.txt is this script's output on an MI355X):

* the worst ratio error / tol of the device and of the oracle per regime of tau, tol = LNL_RTOL |L| + 2^-53 G, over every point
  of every block of the test's cases, against exact arithmetic (tests/f81_exact_ref.py);
* whether the device's e = exp(-mu t') has the bits of numpy.exp at small arguments (through Engine.pij of a two-state JC
  model: mu = 2 and P_01 = (1 - e) / 2 are exact there, so e = 1 - 2 P_01);
* for tau = 0 -> 1e-8, the tau component of the forward-difference gradient by device, oracle and exact arithmetic.

    python scripts/optimiser_points_report.py [--commit HASH]
"""
import argparse
import os
import sys
from decimal import Decimal

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

import f81_exact_ref as exact   # noqa: E402
import optimiser_point_cases as cases   # noqa: E402
from oracle import pastml_oracle as orc   # noqa: E402
from pastml_amd import hip   # noqa: E402

LNL_RTOL = 1e-11
# LEVEL_SCHEDULE of tests/test_gpu_parity.py, and no single-launch kernel for small forests
LEVELS = dict(BLOCK_NODES=0, SMALL_MANY_NODES=0, SUPER_MIN=1, STACK_MIN=1, SMALL_MAX_NODES=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    args = ap.parse_args()
    try:
        import torch
        device = '{} ({})'.format(torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName)
    except Exception:   # noqa
        device = 'device 0'
    flat, stats = cases.forest()
    avg = stats.avg_nonzero_brlen
    print('optimiser points: device and oracle against exact arithmetic (60-digit decimal)')
    print('commit {}, {}, library digest {}'.format(args.commit, device, hip.build_digest()))
    print('forest: {} nodes, {} tips, 2 trees, {} zero-length branches; avg non-zero branch {:.6g}'
          .format(flat.n_nodes, flat.n_tips, int(((flat.dist == 0) & (flat.parent >= 0)).sum()), avg))
    print()
    print('1. worst error / tol per regime of tau (zero: tau = 0; tiny: the 1e-8 step next to 0; small: 1e-3 avg and its steps; '
          'large: avg and its steps)')
    gradients = []
    for k, family, shape in [c + ('random',) for c in cases.CASES] + [c + ('clumps',) for c in cases.CLUMP_CASES]:
        b = cases.build(k, family, shape)
        flat, stats = b['flat'], b['stats']
        avg = stats.avg_nonzero_brlen
        batch = b['batch']
        w = cases.width(b)
        # (the forest of balanced clumps: through the level launches with their two-level and stacked units, as in the test)
        batch.open_optimiser([w, w], tune=LEVELS if shape == 'clumps' else None)
        worst = {}
        try:
            for sf0, tau0 in cases.base_points(stats):
                for which in ('models', 'smoothing'):
                    blocks = {c: cases.block_at(b[which][c], sf0, tau0) for c in range(2)}
                    got = batch.evaluate_points(blocks)
                    for c in range(2):
                        pi, sf, tau, tf = cases.as_arrays(blocks[c])
                        triple = []
                        for j in range(len(sf)):
                            masks = cases.column_masks(batch, c, tau[j], b['altered'][c])
                            want = cases.exact_value(b, c, masks, pi[j], sf[j], tau[j], tf[j])
                            ref = orc.bottom_up(flat, masks.astype(int), dict(kind=0, pi=pi[j]), sf[j], tau[j], tf[j])['loglik']
                            key = cases.regime(tau[j], avg)
                            w_ = worst.setdefault(key, [0.0, 0.0])
                            w_[0] = max(w_[0], exact.error_ratio(got[c][j], want, LNL_RTOL))
                            w_[1] = max(w_[1], exact.error_ratio(ref, want, LNL_RTOL))
                            triple.append((float(got[c][j]), float(ref), want['loglik']))
                        if which == 'models' and tau0 == 0 and c == 0:
                            # point 0: the base point (tau = 0, altered masks); point 2: its tau step (1e-8, plain masks)
                            assert tau[0] == 0 and tau[2] == 1e-8
                            gradients.append((k, family + (' clumps' if shape == 'clumps' else ''), sf0 * avg,
                                              (triple[2][0] - triple[0][0]) / 1e-8,
                                              (triple[2][1] - triple[0][1]) / 1e-8,
                                              float((triple[2][2] - triple[0][2]) / Decimal(1e-8)), float(triple[0][2])))
        finally:
            batch.close()
        where = ' (forest of balanced clumps, {} nodes)'.format(flat.n_nodes) if shape == 'clumps' else ''
        print('   k = {:3d} {}{}: '.format(k, family, where)
              + '; '.join('{} device {:.3g} oracle {:.3g}'.format(a, *worst[a]) for a in ('zero', 'tiny', 'small', 'large')))
    print()
    print('2. e = exp(-mu t\') of the device (Engine.pij, two-state JC: e = 1 - 2 P_01 exactly) against numpy.exp and the '
          'correctly rounded value')
    ts = np.array([1e-11, 1e-9, 1e-7, 1e-5, 1e-3, 0.1]) / 2   # (e >= 1/2: 1 - e and 1 - 2 P_01 are exact)
    with hip.Engine(flat, 1, 2) as eng:
        eng.set_models([(dict(kind=0, pi=np.array([0.5, 0.5])), (1., 0., 1.))])
        P = eng.pij(ts)
    for t, p in zip(ts, P):
        e_dev = float(1. - 2. * p[0, 1])
        e_np = float(np.exp(-2. * t))
        e_true = exact.branch_exponentials([0.5, 0.5], [t], 1., 0., 1.)[0]
        units = (Decimal(e_dev) - e_true) / Decimal(float(np.spacing(e_np)))
        print('   mu t = {:.0e}: device {!r}, numpy {!r}: {}; device - true = {:+.3f} units in the last place, '
              'numpy - true = {:+.3f}'
              .format(2 * t, e_dev, e_np, 'same bits' if e_dev == e_np else 'DIFFERENT bits', float(units),
                      float((Decimal(e_np) - e_true) / Decimal(float(np.spacing(e_np))))))
    print()
    print('3. tau component of the forward-difference gradient at tau = 0 (step 1e-8), character 0: (ln L(1e-8) - ln L(0)) / 1e-8')
    for k, family, sfa, dev, ref, true, lnl in gradients:
        print('   k = {:3d} {} sf avg = {:<6g} ln L = {:<12.6f} device {!r}  oracle {!r}  exact {!r}  (device - exact {:+.3g}, '
              'oracle - exact {:+.3g}, device - oracle {:+.3g})'.format(k, family, sfa, lnl, dev, ref, true, dev - true, ref - true,
                                                                        dev - ref))


if __name__ == '__main__':
    main()
