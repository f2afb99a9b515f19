"""
TEST INFRASTRUCTURE: designed inputs of select_states_kernel (pml_kernels_misc.h) -- forests of lone tips whose posterior rows are
chosen, not drawn -- and the census of the branch every row takes.  Host arithmetic only: tests/test_select_states_ref.py holds
every case to what tests/test_gpu_select_states.py relies on, so that the GPU file filters and skips nothing.

How a row is designed.  A tree of a single tip is a legal tree, and td_roots_kernel gives it the posterior pi_i mask_i / sum_j pi_j
mask_j: under the F81 model the mask of tip n in column c picks a subset of the column's frequencies and the device renormalises
it.  A column is therefore a pool of k weights laid out as TEMPLATES -- a few adjacent slots with chosen weights -- and every row is
a subset of one template's slots (the rest of the column is masked off: zero padding).  lh_mask restricts a row further without
renormalising, so a sum below 1, and 0, reach the kernel; the joint state of a row is named by a one-hot mask for a joint pass that
runs before the designed masks are set (pml_select_states asks for the joint states of SOME earlier back-trace), so it is free of
the posterior: on the largest entry, on a small one, on one that lh_mask removed.

Two parts per state count, one engine each: 'a' packs the narrow templates (at most k / 2 slots) into as few columns as hold them,
with a column of templates that end at states 67, 131 and k - 1 (kept states on both sides of a mask word's boundary) and the
dyadic columns; 'b' gives every wide template (rows over all k states: the long walks, m* = k - 1 and k, the uniform row) a column
of its own on a handful of tips.  Small k has many columns of two or three states: one pool yields one two-state row.

Templates (weights are Fractions, scaled to integers; the builder VERIFIES what a row does with tests/select_states_ref.py, the
formulas below only aim):
    dom2 / domM   the largest share s at 0.70, 0.74, 0.75 -+ 2^-40, 0.755, 0.76 -+ 2^-40, 0.80, 0.999 in a row of two states and of
                  up to seven (the rest split unevenly); 0.75 -+ 2^-40 with two states has f(2) - f(1) = 2^-39, between a decided
                  row and a tie, and is left out.  The joint state once on the largest entry and once on a small one.
    early(m)      m nearly equal heads and a tail of 1 / (4 (m + 1)) of the mass: m* = m and the walk's early stop fires at m*.
    eager(m)      m* = m with f(m - 1) just above the bound -1 / m at which the walk may stop after m - 1 candidates and below the
                  -1 / (m + 1) of a stop one candidate too eager ('guard' in the census): such a stop would miss m*.
    late(m)       k states: m equal heads of (1 + a m) / (2 m), a flat tail, a = 1.02 / k: f(m*) = -a lies just below f(k) = -1 / k,
                  so m* = m and the stop fires only near 0.98 k.  (f(k) = -1 / k for every row, so a decided row with m* < k always
                  stops before k: the walk runs TO k only with m* = k.)
    uniform(u)    u equal states (m* = u; MAP: the first of equal maxima), also over all k states.
    run           two large states and a run of up to ten equal small ones.  Inside a run of equal values f is monotone, so a
                  decided m* never cuts a run by itself; with force_joint and the joint state inside the run it does: the joint
                  entry is counted first, m* = 3, and the kept set is the two large states and the run's LOWEST index, not the
                  joint state (ml.py:562-565).
    restricted    lh_mask removes the second state (sum < 1), the joint state (l_last = 0), all but a dominant pair, everything
                  (sum = 0, empty words), or exactly the allowed states (sum = 0 with bits set); wide: every other state of k.
    dyadic        columns whose frequencies are integers / 2^E with sum exactly 1 and whose rows' sums are powers of two, so the
                  device's division is exact and the rows arrive bit for bit: (1/2, 1/4, 1/8, 1/8) with f(2) = f(3) = f(4),
                  (3/4, 1/4) with f(1) = f(2), and (7/8, 1/16, 1/16) on the other side of the 0.76 shortcut (f(2) = f(3) there, m*
                  = 1 decided); with lh_mask (1/2, 0, 1/8, 1/8) has f(1) = f(2) = f(3).  Copies across states 62 .. 65 and 127 / 128.

Every (row, force_joint, lh_mask on / off) is DECIDED (exact gap >= 1e-10; the kernel's rounding of sum and L_m is below 3 k 2^-53
<= 1.8e-13), an exact TIE (gap 0, every value a dyadic the double arithmetic keeps), or ZERO (sum = 0); build() asserts that none
lies in between, that no row is within 2^-42 of the shortcut's 0.76 or of the early stop's bound, and the census.
"""
import functools
import math
from collections import Counter
from fractions import Fraction

import numpy as np

import select_states_ref as ref
from pastml_amd.tree import FlatForest, TreeNode

STATE_COUNTS = (2, 3, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512)
PARTS = ('a', 'b')
CASES = [(k, p) for k in STATE_COUNTS for p in PARTS]
DECIDED = Fraction(1, 10 ** 10)
MARGIN = Fraction(1, 2 ** 42)
E40 = Fraction(1, 2 ** 40)
SHARES = (('0.70', Fraction(7, 10)), ('0.74', Fraction(74, 100)), ('0.75-', Fraction(3, 4) - E40), ('0.75+', Fraction(3, 4) + E40),
          ('0.755', Fraction(755, 1000)), ('0.76-', Fraction(76, 100) - E40), ('0.76+', Fraction(76, 100) + E40),
          ('0.80', Fraction(4, 5)), ('0.999', Fraction(999, 1000)))
N_MIN = {'a': 203, 'b': 9}     # lone tips per part (odd: the last wave of a launch is partly filled wherever a wave holds several)
WORD_ENDS = (68, 132)          # templates ending here keep states on both sides of 63 / 64 and 127 / 128


def lane_shape(k):
    """(G, R) of dispatch_select (pml_launch_matrix.hip)."""
    if k <= 64:
        g = 1
        while g * 8 < k:
            g *= 2
        return g, 8
    return (64, 2) if k <= 128 else (64, 4) if k <= 256 else (64, 8)


def wanted_m(k):
    return sorted({m for m in (1, 2, 3, 7, 8, 9, 16, k - 1, k) if 1 <= m <= k})


# ---------------------------------------------------------------------------------------------------------------------
# templates
# ---------------------------------------------------------------------------------------------------------------------
def _ints(weights):
    fr = [Fraction(x) for x in weights]
    D = 1
    for x in fr:
        D = D * x.denominator // math.gcd(D, x.denominator)
    return [int(x * D) for x in fr]


def template(name, weights, rows, end=None, dyadic=False):
    """rows: (mask slots, lh_mask slots or None = every state, joint slot)."""
    w = list(weights) if dyadic else _ints(weights)
    assert all(x > 0 for x in w)
    return dict(name=name, w=w, rows=[(tuple(sorted(s)), None if lh is None else tuple(sorted(lh)), j) for s, lh, j in rows],
                end=end, dyadic=dyadic)


def dom2(name, s):
    return template('dom2:' + name, [s, 1 - s], [((0, 1), None, 0), ((0, 1), None, 1)])


def dom_many(name, s, t, wide=False):
    parts = [t + 1 + i for i in range(t)]
    w = [s] + [(1 - s) * Fraction(p, sum(parts)) for p in parts]
    every = range(t + 1)
    return template(('domW:' if wide else 'domM:') + name, w, [(every, None, 0), (every, None, 1)])


def early(m, t, reverse=False, end=None):
    head = [1 + Fraction(i, 64 * m ** 3) for i in range(m)]
    eps = Fraction(1, 4 * (m + 1))
    tail_total = sum(head) * eps / (1 - eps)
    tail = [tail_total * Fraction(p, sum(range(2, 2 + t))) for p in range(2, 2 + t)]
    w = head + tail
    joints = [0] + ([m] if t else [])
    if reverse:
        w = w[::-1]
        joints = [len(w) - 1 - j for j in joints]
    return template('early:{}'.format(m), w, [(range(len(w)), None, j) for j in joints], end=end)


def late(m, k):
    a = Fraction(102, 100 * k)
    w = [(1 + a * m) / (2 * m)] * m + [(1 - a * m) / (2 * (k - m))] * (k - m)
    return template('late:{}'.format(m), w, [(range(k), None, 0), (range(k), None, k - 1)])


def eager(m, k):
    """m* = m + 1 with f(m) = -(1 - d) / (m + 1), d = 1 / (4 (m + 2)): just short of the bound -1 / (m + 1) at which the walk may
    stop after m candidates, and below the -1 / (m + 2) of a stop that is one candidate too eager."""
    d = Fraction(1, 4 * (m + 2))
    h = (1 + Fraction(m, m + 1) * (1 - d)) / (2 * m)
    rest = 1 - m * h
    x = rest if m + 2 > k else (1 - d) / (2 * (m + 1)) + d / 4
    w = [h] * m + [x] + ([rest - x] if rest > x else [])
    return template('eager:{}'.format(m + 1), w, [(range(len(w)), None, 0), (range(len(w)), None, len(w) - 1)])


def uniform(u, wide=False):
    rows = [(range(u), None, 0), (range(u), None, u - 1)]
    if u >= 5:
        rows.append((range(1, 4), None, 2))
    return template(('uniformW:' if wide else 'uniform:') + str(u), [1] * u, rows)


def run(r):
    e = Fraction(1, 2 * (4 + 2 * r))
    big = 1 - r * e
    w = [big * Fraction(8, 15), big * Fraction(7, 15)] + [e] * r
    every = range(r + 2)
    return template('run:{}'.format(r), w, [(every, None, 0), (every, None, r + 1), (every, None, 2), (every, None, 2 + r // 2)])


def restricted(width):
    w = [Fraction(x, 100) for x in (41, 29, 15, 10, 3, 2)][:width]
    A = set(range(width))
    last = width - 1
    few = {0, 1} if width > 2 else {0}
    rows = [(A, A - {1}, 0), (A, A - {1}, 1), (A, {0, last}, 0), (A, {0, last}, last), (A, (), 0), (few, A - few, 0),
            (A, A - {0}, 0)]
    return template('restricted:{}'.format(width), w, rows)


def restricted_wide(k):
    w = [3 * k - i for i in range(k)]
    A = range(k)
    return template('restrictedW', w, [(A, range(0, k, 2), 0), (A, range(0, k, 2), 1), (A, (), k - 1), (range(k // 2), range(k // 2, k), 0),
                                       (A, range(k - 3, k), k - 1)])


def dyadic_templates():
    d1 = template('dyadic:1/2,1/4,1/8,1/8', [4, 2, 1, 1], [(range(4), None, 0), (range(4), None, 3), (range(4), None, 2),
                                                           (range(4), (0, 2, 3), 0), (range(4), (0, 2, 3), 1)], dyadic=True)
    d2 = template('dyadic:3/4,1/4', [3, 1], [(range(2), None, 0), (range(2), None, 1)], dyadic=True)
    d3 = template('dyadic:7/8,1/16,1/16', [14, 1, 1], [(range(3), None, 0), (range(3), None, 1)], dyadic=True)
    return d1, d2, d3


def templates(k):
    """(narrow, wide, boundary): the templates of part 'a', those of part 'b', those placed by their last state."""
    out = [dom2(n, s) for n, s in SHARES if not n.startswith('0.75') or n == '0.755']
    if k >= 3:
        out += [dom_many(n, s, min(k - 1, 6)) for n, s in SHARES]
    if k > 14:
        out += [dom_many(n, s, k - 1, wide=True) for n, s in SHARES if n.startswith('0.76')]
    for m in wanted_m(k):
        if m >= 2:
            out.append(early(m, min(3, k - m)))
        if m <= k - 2 and 102 * m < 100 * k and k >= 8:
            out.append(late(m, k))
        if m >= 2:
            out.append(eager(m - 1, k))
    out += [uniform(u) for u in (2, 3, 5, 8, 9, 12) if u < k]
    out.append(uniform(k, wide=True))
    if k >= 4:
        out.append(run(min(10, k - 2)))
    out.append(restricted(min(k, 6)))
    if k >= 8:
        out.append(restricted_wide(k))
    boundary = []
    if k > 64:
        for end in WORD_ENDS + (k,):
            if end <= k and (not boundary or end - 12 >= boundary[-1]['end']):
                boundary.append(early(9, 3, reverse=True, end=end))
    narrow = [t for t in out if 2 * len(t['w']) <= k]
    wide = [t for t in out if 2 * len(t['w']) > k]
    return narrow, wide, boundary


def _is_pow2(x):
    return x > 0 and x & (x - 1) == 0


def dyadic_columns(k):
    """[[(offset, template)]]: the dyadic templates in as few columns as leave a slot for the remainder of 2^E (or fill a column to
    a power of two exactly); the first column also carries the copies across the mask words' boundaries."""
    d1, d2, d3 = dyadic_templates()
    pending = [t for t in (d1, d2, d3) if len(t['w']) <= k]
    cols = []
    while pending:
        placed, cur, units = [], 0, 0
        for t in list(pending):
            w = len(t['w'])
            if cur + w < k or (cur + w == k and _is_pow2(units + sum(t['w']))):
                placed.append((cur, t))
                cur += w
                units += sum(t['w'])
                pending.remove(t)
        assert placed
        if not cols:
            for at, t in ((62, d1), (127, d2), (k - 5, d1)):
                if at >= cur + 1 and at + len(t['w']) < k and all(at >= o + len(p['w']) for o, p in placed):
                    placed.append((at, t))
        cols.append(placed)
    return cols


def pack(narrow, k):
    cols, cur = [[]], 0
    for t in narrow:
        if cur + len(t['w']) > k:
            cols.append([])
            cur = 0
        cols[-1].append((cur, t))
        cur += len(t['w'])
    return [c for c in cols if c]


def layout(k, part):
    """[(kind, [(offset, template)])] per column; kind: 'plain' or 'dyadic'."""
    narrow, wide, boundary = templates(k)
    if part == 'b':
        return [('plain', [(0, t)]) for t in wide]
    cols = [('plain', c) for c in pack(narrow, k)]
    if boundary:
        cols.append(('plain', [(t['end'] - len(t['w']), t) for t in boundary]))
    return cols + [('dyadic', c) for c in dyadic_columns(k)]


def column_weights(k, kind, placed):
    """(integer weights [k], their total): the column's frequencies are weights / total.  plain: every template scaled to the same
    total, the free slots share one more; dyadic: units of 2^-E, the free slots take what is missing to 2^E."""
    w = [0] * k
    free = set(range(k))
    for off, t in placed:
        for i in range(len(t['w'])):
            assert off + i in free, 'templates overlap'
            free.discard(off + i)
    free = sorted(free)
    if kind == 'dyadic':
        for off, t in placed:
            w[off:off + len(t['w'])] = t['w']
        units = sum(w)
        total = 1
        while total < units + len(free):
            total *= 2
        for n, i in enumerate(free):
            w[i] = total - units - (len(free) - 1) if n == 0 else 1
        assert sum(w) == total and _is_pow2(total) and total < 2 ** 50
        return w, total
    common = 1
    for _, t in placed:
        s = sum(t['w'])
        common = common * s // math.gcd(common, s)
    common *= max(1, len(free))
    for off, t in placed:
        scale = common // sum(t['w'])
        w[off:off + len(t['w'])] = [x * scale for x in t['w']]
    for i in free:
        w[i] = common // len(free)
    return w, sum(w)


# ---------------------------------------------------------------------------------------------------------------------
# what a row does, from the inputs alone
# ---------------------------------------------------------------------------------------------------------------------
def describe(v, joint):
    """The exact selection of the integer row v (joint: index or None) and the kernel's branch in exact arithmetic:
    dict(kind 'decided' | 'tie' | 'zero', m, kept, gap, branch 'scan' | 'shortcut' | 'walk', stop (the candidate the walk ends at), path
    'one' | 'butterfly' | 'ranks')."""
    k = len(v)
    r = ref.select_mppa(v, joint)
    out = dict(m=r['m'], kept=r['kept'], gap=r['gap'], stop=None)
    S = sum(v)
    if S == 0:
        out.update(kind='zero', branch='scan')
    else:
        if r['gap'] is None or r['gap'] >= DECIDED:
            out['kind'] = 'decided'
        else:
            assert r['gap'] == 0, 'a row between decided and tied: gap {}'.format(float(r['gap']))
            out['kind'] = 'tie'
        l_last = v[joint] if joint is not None else max(v)
        assert abs(Fraction(l_last, S) - Fraction(76, 100)) >= MARGIN, 'a row at the 0.76 shortcut'
        if 100 * l_last >= 76 * S:
            out['branch'] = 'shortcut'
            assert r['m'] == 1, 'the shortcut is wrong'
        else:
            out['branch'] = 'walk'
            order = ref._walk_sums(v, joint)
            L, best_num, best_m = 0, None, k
            for m in range(1, k + 1):
                L += v[order[m - 1]]
                num = S - 2 * L
                if best_num is None or num * best_m < best_num * m:
                    best_num, best_m = num, m
                # best_f < -(1 + 1e-9) S / (m + 1), with the margin that keeps the double arithmetic on the same side
                lhs = Fraction(best_num, best_m * S) + (1 + Fraction(1, 10 ** 9)) / (m + 1)
                if m < r['m'] and Fraction(best_num, best_m * S) + Fraction(1, m + 2) < -MARGIN:
                    out['guard'] = True   # (a stop after m candidates at -S / (m + 2) would miss m*)
                assert abs(lhs) >= MARGIN, 'a row at the early stop'
                out['stop'] = m
                if lhs < 0:
                    break
            assert best_m == r['m'], 'the early stop is wrong'
    out['path'] = 'one' if out['m'] == 1 else 'butterfly' if out['m'] <= 8 else 'ranks'
    return out


def _labels(k, t, row, d, fj, lh_on, v_mask, v, joint_abs):
    """Census keys of one (row, force_joint, lh_mask on / off)."""
    keys = [d['kind'], d['branch'], 'path:' + d['path']]
    name = t['name']
    if d['branch'] == 'walk':
        m, stop = d['m'], d['stop']
        when = 'early' if stop == m else 'late' if stop >= max(m + 1, (9 * k) // 10) else 'mid'
        keys.append('walk:m={}:{}'.format(m, when))
        if stop == k:
            keys.append('walk:to_k')
        if d.get('guard'):
            keys.append('walk:m={}:guard'.format(m))
    if name.startswith('dom') and not lh_on:
        keys.append('{}:{}'.format(name, 'joint_small' if fj and v[joint_abs] != max(v) else 'plain'))
    if fj and sum(v) > 0:
        if v[joint_abs] == 0:
            keys.append('joint_removed' if v_mask[joint_abs] else 'joint_outside')
        elif v[joint_abs] != max(v):
            keys.append('joint_not_largest')
    if lh_on and 0 < sum(v) < sum(v_mask):
        keys.append('sum<1')
    if d['kind'] == 'zero':
        keys.append('scan:lh_empty' if row[1] == () else 'scan:lh_bits')
    kept = set(d['kept'])
    if sum(v) > 0:
        for a in (63, 127):
            if a in kept and a + 1 in kept:
                keys.append('kept:{}/{}'.format(a, a + 1))
        if k - 1 in kept and k > 64:
            keys.append('kept:k-1')
        top = sorted(v, reverse=True)
        if d['m'] < k and top[d['m'] - 1] == top[d['m']] and top[d['m']] > 0:
            keys.append('kept_cuts_equal_values')
        if len([x for x in v if x == top[0]]) > 1:
            keys.append('map_tie')
        if name.startswith(('uniform', 'run', 'late')):
            keys.append('value_ties')
        if t['dyadic']:
            keys.append('dyadic:' + d['branch'])
    return keys


def wanted(k):
    """The census keys a state count must show (both parts together)."""
    want = {'decided', 'tie', 'zero', 'scan', 'shortcut', 'walk', 'path:one', 'path:butterfly', 'sum<1', 'joint_removed',
            'joint_not_largest', 'scan:lh_empty', 'scan:lh_bits', 'value_ties', 'map_tie', 'walk:to_k', 'dyadic:walk'}
    for n, _ in SHARES:
        if not n.startswith('0.75') or n == '0.755':
            want |= {'dom2:{}:plain'.format(n), 'dom2:{}:joint_small'.format(n)}
        if k >= 3:
            want |= {'domM:{}:plain'.format(n), 'domM:{}:joint_small'.format(n)}
    for m in wanted_m(k):
        want.add('walk:m={}:early'.format(m))
        if m >= 2:
            want.add('walk:m={}:guard'.format(m))
        if m <= k - 2 and 102 * m < 100 * k and k >= 8:
            want.add('walk:m={}:late'.format(m))
    if k >= 3:
        want.add('dyadic:shortcut')
    if k >= 4:
        want.add('kept_cuts_equal_values')
    if k >= 9:
        want.add('path:ranks')
    if k > 64:
        want |= {'kept:63/64', 'kept:k-1'}
    if k >= 132:
        want.add('kept:127/128')
    return want


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
CONFIGS = [(fj, lh) for fj in (False, True) for lh in (False, True)]


@functools.lru_cache(maxsize=None)
def build(k, part, n_min=None):
    """
    dict(k, part, flat, C, N, pi [C, k], weights (integers [C][k]), masks, lh_masks, joint_masks int8 [C, N, k], joint [C, N],
    dyadic [C] bool, rows [C][N] (offset, template, row), n_designed [C] (the tips before the rows repeat), exact {(fj, lh): [C][N] describe()}, census Counter, min_gap Fraction) or None
    where a part is empty.  n_min: at least that many lone tips (the rows repeat in turn).
    """
    cols = layout(k, part)
    if not cols:
        return None
    C = len(cols)
    per_col = [[(off, t, row) for off, t in placed for row in t['rows']] for _, placed in cols]
    N = max(max(len(r) for r in per_col), n_min or N_MIN[part]) | 1
    flat = FlatForest.from_trees([TreeNode(name='t{}'.format(i), dist=0.0) for i in range(N)])
    assert flat.n_nodes == N and len(flat.roots) == N
    pi = np.zeros((C, k))
    weights = []
    masks = np.zeros((C, N, k), dtype=np.int8)
    lh_masks = np.ones((C, N, k), dtype=np.int8)
    joint_masks = np.zeros((C, N, k), dtype=np.int8)
    joint = np.zeros((C, N), dtype=np.int64)
    exact = {cfg: [[None] * N for _ in range(C)] for cfg in CONFIGS}
    census = Counter()
    min_gap = None
    rows = []
    for c, (kind, placed) in enumerate(cols):
        w, total = column_weights(k, kind, placed)
        weights.append(w)
        pi[c] = [float(Fraction(x, total)) for x in w]
        if kind == 'dyadic':
            assert all(Fraction(float(p)) == Fraction(x, total) for p, x in zip(pi[c], w)) and math.fsum(pi[c]) == 1.0
        rows.append([per_col[c][n % len(per_col[c])] for n in range(N)])
        seen = {}
        for n, (off, t, row) in enumerate(rows[c]):
            sub, lh, j = row
            for s in sub:
                masks[c, n, off + s] = 1
            if lh is not None:
                lh_masks[c, n] = 0
                for s in lh:
                    lh_masks[c, n, off + s] = 1
            joint[c, n] = off + j
            joint_masks[c, n, off + j] = 1
            key = n % len(per_col[c])
            if key not in seen:
                v_mask = [w[i] if masks[c, n, i] else 0 for i in range(k)]
                v_lh = [x if lh_masks[c, n, i] else 0 for i, x in enumerate(v_mask)]
                if kind == 'dyadic':
                    assert _is_pow2(sum(v_mask)), 'a dyadic row whose sum is no power of two'
                seen[key] = {}
                for fj, lh_on in CONFIGS:
                    v = v_lh if lh_on else v_mask
                    d = describe(v, int(joint[c, n]) if fj else None)
                    assert d['kind'] != 'tie' or kind == 'dyadic', 'a tie outside the dyadic columns: {} {} {} {}'.format(t['name'], row, fj, lh_on)
                    seen[key][fj, lh_on] = (d, _labels(k, t, row, d, fj, lh_on, v_mask, v, int(joint[c, n])))
            for cfg in CONFIGS:
                d, keys = seen[key][cfg]
                exact[cfg][c][n] = d
                if n < len(per_col[c]):   # (the census counts designed rows, not their repeats)
                    census.update(keys)
                    if d['kind'] == 'decided' and d['gap'] is not None:
                        min_gap = d['gap'] if min_gap is None else min(min_gap, d['gap'])
    assert masks.sum(axis=2).min() >= 1
    for a in (pi, masks, lh_masks, joint_masks, joint):
        a.setflags(write=False)
    return dict(k=k, part=part, flat=flat, C=C, N=N, pi=pi, weights=weights, masks=masks, lh_masks=lh_masks, joint_masks=joint_masks,
                joint=joint, dyadic=np.array([kind == 'dyadic' for kind, _ in cols]), rows=rows, exact=exact, census=census,
                min_gap=min_gap, n_designed=[len(r) for r in per_col])


def specs_of(b):
    """The columns' models as Engine.set_models takes them: F81, scaling factor 1."""
    return [(dict(kind=0, pi=b['pi'][c]), (1.0, 0.0, 1.0)) for c in range(b['C'])]


def ideal_posteriors(b):
    """[C, N, k]: pi mask / sum in numpy doubles, what td_roots_kernel computes up to the order of the sum."""
    lh = b['pi'][:, None, :] * b['masks']
    return lh / lh.sum(axis=2, keepdims=True)


def designed_posteriors(b, c):
    """[N, k] of a dyadic column: the designed values, converted exactly."""
    out = np.zeros((b['N'], b['k']))
    for n in range(b['N']):
        v = [x if m else 0 for x, m in zip(b['weights'][c], b['masks'][c, n])]
        S = sum(v)
        for i, x in enumerate(v):
            q = Fraction(x, S)
            out[n, i] = float(q)
            assert Fraction(out[n, i]) == q
    return out


def census_of(k):
    total = Counter()
    for part in PARTS:
        b = build(k, part)
        if b is not None:
            total.update(b['census'])
    return total


# ---------------------------------------------------------------------------------------------------------------------
# the record: `PYTHONPATH=. python tests/select_states_cases.py` prints what profiles/select_states_exact.txt holds below its heading
# ---------------------------------------------------------------------------------------------------------------------
def tie_answers(b):
    """[(column, node, force_joint, lh_mask, template, m of ml.select_mppa, exact m)] of every designed exact tie of a case, on
    the rows numpy computes: what the float64 restatement answers where only exact arithmetic can name the first minimiser."""
    from pastml_amd import ml
    post = ideal_posteriors(b)
    out = []
    for c in np.flatnonzero(b['dyadic']):
        for fj, lh_on in CONFIGS:
            lh = post[c] * b['lh_masks'][c] if lh_on else post[c]
            with np.errstate(invalid='ignore', divide='ignore'):
                _, host_k = ml.select_mppa(lh, b['joint'][c] if fj else None)
            for n in range(b['n_designed'][c]):
                d = b['exact'][fj, lh_on][c][n]
                if d['kind'] == 'tie':
                    out.append((int(c), n, fj, lh_on, b['rows'][c][n][1]['name'], int(host_k[n]), d['m']))
    return out


def report():
    """The census per state count, the smallest exact gap of the decided rows, and the exact ties on which ml.select_mppa does not
    answer the first minimiser, as lines of text."""
    import textwrap
    out = []
    P = out.append
    P('Per state count, both parts together: designed rows x (force_joint, lh_mask) = 4 configurations each; repeats of a row on')
    P('further tips are not counted.  shape = lane shape G x R of dispatch_select, W = mask words.')
    P('')
    P('   k  shape    W  cols  rows  decided  tie  zero | shortcut  walk  scan | one  butterfly  ranks | early  mid  late  to_k | smallest gap')
    smallest = None
    for k in STATE_COUNTS:
        c = census_of(k)
        bs = [build(k, p) for p in PARTS]
        gap = min(b['min_gap'] for b in bs)
        smallest = gap if smallest is None else min(smallest, gap)

        def walks(when):
            return sum(n for key, n in c.items() if key.startswith('walk:m=') and key.endswith(when))
        P('{:4d}  {:7s} {:2d}  {:4d}  {:4d}  {:7d}  {:3d}  {:4d} | {:8d}  {:4d}  {:4d} | {:3d}  {:9d}  {:5d} | {:5d}  {:3d}  {:4d}  {:4d} | {:.3g}'
          .format(k, '{}x{}'.format(*lane_shape(k)), (k + 63) // 64, sum(b['C'] for b in bs), sum(sum(b['n_designed']) for b in bs),
                  c['decided'], c['tie'], c['zero'], c['shortcut'], c['walk'], c['scan'], c['path:one'], c['path:butterfly'],
                  c['path:ranks'], walks(':early'), walks(':mid'), walks(':late'), c['walk:to_k'], float(gap)))
    P('')
    P('smallest exact gap among the decided rows of all cases: {:.3g} (a decided row: 1e-10 at least; the kernel\'s rounding: 1.8e-13)'
      .format(float(smallest)))
    P('early: the stop fires at m*; late: at 0.9 k or beyond; to_k: the walk takes all k candidates (m* = k); guard: f before m* lies')
    P('below -S / (m + 2), so that a stop one candidate too eager would miss m*.')
    P('')
    P('Tiers per state count (counts of (row, configuration) pairs):')
    for k in STATE_COUNTS:
        c = census_of(k)
        assert not wanted(k) - set(c)
        walk = {}
        for key, n in c.items():
            if key.startswith('walk:m='):
                m, when = key[7:].split(':')
                walk.setdefault(int(m), {})[when] = n
        two = sorted({key.split(':')[1] for key in c if key.startswith('dom2')})
        many = sorted({key.split(':')[1] for key in c if key.startswith('domM')})
        P('  k = {}: dominant {} -- two states at {} shares, many states at {}, each with the joint state on the largest and on a small'
          .format(k, sum(n for key, n in c.items() if key.startswith('dom')), len(two), len(many)))
        P('      entry; value ties {}, kept set cuts equal values {}, MAP ties {}, sum < 1 {}, joint state removed by lh_mask {},'
          .format(c['value_ties'], c['kept_cuts_equal_values'], c['map_tie'], c['sum<1'], c['joint_removed']))
        P('      joint state not the largest {}, sum = 0 with empty lh words {} / with bits {}, dyadic walk {} / shortcut {},'
          .format(c['joint_not_largest'], c['scan:lh_empty'], c['scan:lh_bits'], c['dyadic:walk'], c['dyadic:shortcut']))
        P('      kept across 63/64 {}, 127/128 {}, k-1 {};  walk m*(early/mid/late/guard):'
          .format(c['kept:63/64'], c['kept:127/128'], c['kept:k-1']))
        for line in textwrap.wrap(' '.join('{}({}/{}/{}/{})'.format(m, w.get('early', 0), w.get('mid', 0), w.get('late', 0),
                                                                    w.get('guard', 0)) for m, w in sorted(walk.items())), 118):
            P('        ' + line)
    P('')
    P('Two states at 0.75 -+ 2^-40 are not among the shares: f(2) - f(1) = 2^-39 = 1.8e-12 there, neither a decided row (1e-10) nor a')
    P('tie; the many-state rows carry those two shares (there the runner-up is far).')
    P('')
    P('Exact ties: what the float64 restatement ml.select_mppa answers against the exact first minimiser (recorded, not asserted).')
    P('Rows (k, part, column, node, force_joint, lh_mask) template: its m / exact m')
    n_tie = n_diff = 0
    for k in STATE_COUNTS:
        for part in PARTS:
            for c, n, fj, lh_on, name, host_m, m in tie_answers(build(k, part)):
                n_tie += 1
                if host_m != m:
                    n_diff += 1
                    P('  ({}, {}, {}, {}, {}, {})  {}: {} / {}'.format(k, part, c, n, fj, lh_on, name, host_m, m))
    P('{} tie rows x configurations, {} where ml.select_mppa differs'.format(n_tie, n_diff))
    return out


if __name__ == '__main__':
    print('\n'.join(report()))
