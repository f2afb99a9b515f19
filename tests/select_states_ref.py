"""
TEST INFRASTRUCTURE: the MPPA / MAP state selection (pastml/ml.py:505-595) in exact arithmetic, for the rows on which
tests/test_select_states_ref.py and tests/test_gpu_select_states.py hold ml.select_mppa and select_states_kernel.

Plain Python integers.  Every double of a likelihood row is a dyadic rational (float.as_integer_ratio); the row is scaled to its
common denominator, so that sums, differences and the cross-multiplied comparisons below are integer operations: nothing is
rounded.  With S the sum of the row, L_m the sum of its m largest entries -- the joint state's entry taken first where one is
given -- the reference's criterion is

    sum_i (u_m[i] - q[i])^2 = sum_i q_i^2 + (1 - 2 L_m / S) / m,      u_m = (0, .., 0, 1/m x m), q the sorted probabilities,

so its first minimiser is the first minimiser of f(m) = (S - 2 L_m) / m; f(a) < f(b) is (S - 2 L_a) b < (S - 2 L_b) a.
criterion_by_fractions evaluates the left-hand side directly, as the reference writes it, for the host test of that identity.

The kept states are the m* largest entries, ties to the lower index (ml.py:562-565: the sort key's first component is constant,
so the joint state is NOT forced in -- the behaviour of the reference, of ml.select_mppa and of the kernel).  A row of zeros
keeps every state (the reference's NaN probabilities never compare below the initial best value, so m stays k).
"""
import math
from fractions import Fraction


def exact_ints(row):
    """(integers v, D) with row[i] == v[i] / D exactly; the entries must be finite."""
    ratios = [float(x).as_integer_ratio() for x in row]
    D = max(d for _, d in ratios)
    return [n * (D // d) for n, d in ratios], D


def _walk_sums(v, joint):
    """The states in the order the criterion takes them: the joint state, then by descending value.  (Which of equal values comes
    first does not change a sum.)"""
    order = sorted(range(len(v)), key=lambda i: (-v[i], i))
    if joint is not None:
        order.remove(joint)
        order.insert(0, joint)
    return order


def select_mppa(row, joint=None):
    """
    dict(m: the exact first minimiser of f, gap: min over m' != m of (f(m') - f(m)) / S as a Fraction (None for a row of zeros or of
    one state), kept: the sorted indices of the kept states, S: the row's sum as a Fraction).
    `row` may hold doubles, or integers or Fractions (an ideal row): Fractions are scaled to a common denominator the same way.
    """
    if all(isinstance(x, int) for x in row):
        v, D = list(row), 1
    elif all(isinstance(x, float) for x in row):
        v, D = exact_ints(row)
    else:
        fr = [Fraction(x) for x in row]
        D = 1
        for x in fr:
            D = D * x.denominator // math.gcd(D, x.denominator)
        v = [int(x * D) for x in fr]
    k = len(v)
    assert all(x >= 0 for x in v)
    if joint is not None:
        joint = int(joint)
        assert 0 <= joint < k
    S = sum(v)
    by_value = sorted(range(k), key=lambda i: (-v[i], i))
    if S == 0:
        return dict(m=k, gap=None, kept=list(range(k)), S=Fraction(0))
    order = _walk_sums(v, joint)
    # f(m) = num[m] / m.  Once L_m = S every later f is -S / m', which rises with m': the minimum and the runner-up lie at or before
    # the first m' after that point, so the loop ends there.
    nums = []
    L = 0
    for m in range(1, k + 1):
        full = L == S
        L += v[order[m - 1]]
        nums.append(S - 2 * L)
        if full:
            break
    best = 1
    for m in range(2, len(nums) + 1):
        if nums[m - 1] * best < nums[best - 1] * m:   # strict: the first minimiser
            best = m
    gap = None   # (d, m'): f(m') - f(best) = d / (m' best), the smallest over m'
    for m in range(1, len(nums) + 1):
        if m == best:
            continue
        d = nums[m - 1] * best - nums[best - 1] * m
        assert d >= 0
        if gap is None or d * gap[1] < gap[0] * m:
            gap = (d, m)
    return dict(m=best, gap=None if gap is None else Fraction(gap[0], gap[1] * best * S), kept=sorted(by_value[:best]),
                S=Fraction(S, D))


def select_map(row):
    """The first maximum."""
    row = list(row)
    return max(range(len(row)), key=lambda i: (row[i], -i))


def criterion_by_fractions(row, joint=None):
    """[sum_i (u_m[i] - q[i])^2 for m = 1 .. k] as the reference computes it (ml.py:546-560), in Fractions: the probabilities
    sorted ascending, the joint state's moved last."""
    p = [Fraction(x) for x in row]
    S = sum(p)
    p = [x / S for x in p]
    k = len(p)
    rest = sorted(x for i, x in enumerate(p) if i != joint)
    q = rest + ([p[joint]] if joint is not None else [])
    out = []
    for m in range(1, k + 1):
        u = [Fraction(0)] * (k - m) + [Fraction(1, m)] * m
        out.append(sum((a - b) ** 2 for a, b in zip(u, q)))
    return out


def f_values(row, joint=None):
    """[f(m) / S for m = 1 .. k] as Fractions, every m (no early end): what criterion_by_fractions is compared with."""
    p = [Fraction(x) for x in row]
    S = sum(p)
    order = _walk_sums(p, joint)
    out, L = [], Fraction(0)
    for m in range(1, len(p) + 1):
        L += p[order[m - 1]]
        out.append((S - 2 * L) / (m * S))
    return out
