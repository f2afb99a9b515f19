"""
TEST INFRASTRUCTURE: the marginal pass (and, on request, the joint bottom-up sweep) of a model given by its transition operator --
the eigen models (JTT, CUSTOM_RATES) and HKY -- restated in Python's ``decimal`` at 50 digits with unbounded exponents.

As in tests/f81_exact_ref.py nothing is rounded to a double and nothing is rescaled: the inputs are the doubles the device is
handed (``pi``, ``d``, ``A``, ``Ainv``, ``kappa``, ``sf``, ``tau``, ``tf``), converted exactly (``Decimal(float)``); what is
computed is the value the sweeps would give in exact arithmetic ON THOSE INPUTS -- the rounding numpy left in A and A^-1 is part
of the model here, as it is for the device -- and the only error is that of 50-digit arithmetic.

    t'      = (d_n + tau) tf sf                               (pastml/models/__init__.py:269-270)
    eigen:  P(t') v = A (e o (A^-1 v)),  e = exp(d t')        (generator.py:54-65; P(t') itself only on request, ``pij``)
    HKY:    P(t') in closed form                              (HKYModel.py:55-82, as oracle/pastml_oracle.py:84-113 restates it)
    message = P v_n
    v_p     = mask_p * prod over the children n of p of message_n          (ml.py:82-148, marginal)
    L_tree  = pi . v_root
    down_n  = P_n x,  x = down_p * v_p / message_n;  down_root = 1         (ml.py:240-290)
    lh_n    = v_n * down_n * pi * mask_n,  posterior_n = lh_n / sum(lh_n)  (ml.py:454-460, 498-500)

Children have larger ids than their parents in a FlatForest, so ``reversed(range(N))`` is a bottom-up order.
"""
import decimal
from decimal import Decimal

import numpy as np

DIGITS = 50
_CONTEXT = decimal.Context(prec=DIGITS, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
ZERO, ONE = Decimal(0), Decimal(1)
MINUS_INFINITY = Decimal('-Infinity')
LOG2_OF_10 = float(np.log2(10.))

KIND_HKY, KIND_EIGEN = 1, 2


def _dec_array(a):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        assert not a.imag.any(), 'a complex eigen-decomposition has no restatement here'
        a = a.real
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(*a.shape):
        out[idx] = Decimal(float(a[idx]))
    return out


def _ln(x):
    return x.ln() if x > 0 else MINUS_INFINITY


def log10_float(x):
    """log10 of a Decimal as a float: the decimal exponent plus log10 of the mantissa in float64 -- good to 1e-15 absolute plus
    the spacing of the result, without decimal's own logarithm, which would cost more than the pass.  -inf for 0, nan below."""
    if x == 0:
        return -np.inf
    if x < 0:
        return np.nan
    e = x.adjusted()
    return e + float(np.log10(float(x.scaleb(-e))))


def _log10_rows(rows):
    return np.array([[log10_float(x) for x in row] for row in rows])


class EigenOperator(object):
    """P(t'_n) v = A (e_n o (A^-1 v)) for the branch above node n."""

    def __init__(self, spec, dist, sf, tau, tf):
        self.k = len(spec['pi'])
        self.A, self.Ainv, self.d = _dec_array(spec['A']), _dec_array(spec['Ainv']), _dec_array(spec['d'])
        scale = Decimal(float(tf)) * Decimal(float(sf))
        tau = Decimal(float(tau))
        self.t = [(Decimal(float(x)) + tau) * scale for x in dist]
        self._e = {}

    def exponentials(self, n):
        if n not in self._e:
            self._e[n] = np.array([(x * self.t[n]).exp() for x in self.d], dtype=object)
        return self._e[n]

    def apply(self, n, v):
        nz = [i for i, x in enumerate(v) if x != 0]
        if len(nz) * 4 < self.k:   # (an observed tip: a column of A^-1 instead of the whole product)
            z = self.Ainv[:, nz].dot(v[nz])
        else:
            z = self.Ainv.dot(v)
        return self.A.dot(self.exponentials(n) * z)

    def pij(self, n):
        return (self.A * self.exponentials(n)[None, :]).dot(self.Ainv)

    def pij_columns(self, n, cols):
        return (self.A * self.exponentials(n)[None, :]).dot(self.Ainv[:, cols])

    def pij_row(self, n, i):
        return (self.A[i] * self.exponentials(n)).dot(self.Ainv)


class HKYOperator(object):
    """P(t') of HKY (states A C G T) in closed form, entry by entry as HKYModel.py:55-82 writes it."""

    def __init__(self, spec, dist, sf, tau, tf):
        self.k = 4
        self.pi = _dec_array(spec['pi'])
        self.kappa = Decimal(float(spec['kappa']))
        scale = Decimal(float(tf)) * Decimal(float(sf))
        tau = Decimal(float(tau))
        self.t = [(Decimal(float(x)) + tau) * scale for x in dist]
        self._p = {}

    def pij(self, n):
        if n in self._p:
            return self._p[n]
        pi, kappa, tt = self.pi, self.kappa, self.t[n]
        a, c, g, t = pi
        ag, ct = a + g, c + t
        beta = ONE / (2 * (ag * ct + kappa * (a * g + c * t)))
        eb = (-beta * tt).exp()
        e_ct = (-beta * tt * (ONE + ct * (kappa - ONE))).exp() / ct
        e_ag = (-beta * tt * (ONE + ag * (kappa - ONE))).exp() / ag
        s_ct = (ct + ag * eb) / ct
        s_ag = (ag + ct * eb) / ag
        p = np.empty((4, 4), dtype=object)
        for i in range(4):
            for j in range(4):
                p[i, j] = (ONE - eb) * pi[j]
        p[3, 3] = t * s_ct + c * e_ct
        p[3, 1] = c * s_ct - c * e_ct
        p[1, 3] = t * s_ct - t * e_ct
        p[1, 1] = c * s_ct + t * e_ct
        p[0, 0] = a * s_ag + g * e_ag
        p[0, 2] = g * s_ag - g * e_ag
        p[2, 0] = a * s_ag - a * e_ag
        p[2, 2] = g * s_ag + a * e_ag
        self._p[n] = p
        return p

    def pij_columns(self, n, cols):
        return self.pij(n)[:, cols]

    def pij_row(self, n, i):
        return self.pij(n)[i]

    def apply(self, n, v):
        return self.pij(n).dot(v)


def operator(spec, dist, sf=1., tau=0., tf=1.):
    kind = spec['kind']
    if kind == KIND_EIGEN:
        return EigenOperator(spec, dist, sf, tau, tf)
    if kind == KIND_HKY:
        return HKYOperator(spec, dist, sf, tau, tf)
    raise ValueError('no exact restatement of model kind {} here (the F81 family: tests/f81_exact_ref.py)'.format(kind))


def pij(spec, t, sf=1., tau=0., tf=1.):
    """P(t') of one branch length as a k x k object array of Decimals."""
    with decimal.localcontext(_CONTEXT):
        return operator(spec, [t], sf, tau, tf).pij(0)


def _ratio(vec, worst):
    hi = max(vec)
    r = min(vec) / hi if hi > 0 else ZERO
    return r if worst is None or r < worst else worst


def marginal_pass(flat, masks, spec, sf=1., tau=0., tf=1., top_down=True):
    """
    flat: parent / first_child / n_children / dist / roots (pastml_amd.tree.FlatForest); masks: 0/1 [N, k].
    Returns dict(
        loglik (Decimal, sum over the trees; -Infinity where the likelihood is zero), loglik_per_tree (list of Decimal),
        bu_log10 [N, k] float: log10 of the true bottom-up vectors (-inf for zeros),
        min_message_ratio (float): the smallest entry of a message P v (of P x, top-down) over that vector's largest entry -- while
            it is far above the rounding of float64 no clamp of the sweeps (fmax(., 0); contrib <= 0 -> 1) can have acted,
        and with top_down: td_log10 [N, k], posterior [N, k] (float), lh_log10 [N]: log10 of each node's marginal-likelihood sum
        sum_i v_n[i] down_n[i] pi[i] mask_n[i] (the tree's likelihood, up to what A A^-1 of the given doubles differs from 1)).
    """
    parent, first_child, n_children = flat.parent, flat.first_child, flat.n_children
    N, k = np.asarray(masks).shape
    allowed = np.asarray(masks) != 0
    with decimal.localcontext(_CONTEXT):
        op = operator(spec, flat.dist, sf, tau, tf)
        pi = _dec_array(spec['pi'])
        v = [None] * N
        message = [None] * N
        worst = None
        shared = {}
        for n in reversed(range(N)):
            row = np.array([ONE if a else ZERO for a in allowed[n]], dtype=object)
            fc = int(first_child[n])
            for c in range(fc, fc + int(n_children[n])):
                row = row * message[c]
            v[n] = row
            if parent[n] >= 0:
                # (tips with the same mask on branches of the same length send the same message: computed once)
                key = (op.t[n], allowed[n].tobytes()) if n_children[n] == 0 else None
                if key is None or key not in shared:
                    shared[key] = op.apply(n, row)
                    worst = _ratio(shared[key], worst)
                message[n] = shared[key]
        per_tree = [_ln(pi.dot(v[int(r)])) for r in flat.roots]
        out = dict(loglik=sum(per_tree, ZERO), loglik_per_tree=per_tree, bu_log10=_log10_rows(v))
        if top_down:
            down = [None] * N
            post = np.zeros((N, k))
            lh_log10 = np.zeros(N)
            for n in range(N):   # parents first
                p = int(parent[n])
                if p < 0:
                    down[n] = np.array([ONE] * k, dtype=object)
                else:
                    # (... and such tips of one parent receive the same vector)
                    key = (p, op.t[n], allowed[n].tobytes()) if n_children[n] == 0 else None
                    if key is None or key not in shared:
                        x = np.array([dp * vp / m if vp else ZERO for dp, vp, m in zip(down[p], v[p], message[n])], dtype=object)
                        shared[key] = op.apply(n, x)
                        worst = _ratio(shared[key], worst)
                    down[n] = shared[key]
                lh = v[n] * down[n] * pi   # (v carries the node's mask)
                total = sum(lh, ZERO)
                post[n] = [float(x / total) for x in lh] if total > 0 else np.nan
                lh_log10[n] = log10_float(total)
            out.update(td_log10=_log10_rows(down), posterior=post, lh_log10=lh_log10)
        out['min_message_ratio'] = float(worst) if worst is not None else 1.0
    return out


def joint_pass(flat, masks, spec, sf=1., tau=0., tf=1.):
    """
    The joint (max-product) bottom-up sweep, ml.py:82-148 with is_marginal False, on P(t') built branch by branch, and only in the
    columns j where v_n[j] is not zero (an observed tip: one column): message_n[i] = max_j P_n[i, j] v_n[j].
    Returns dict(loglik (Decimal: sum over the trees of ln max_i pi_i v_root[i]), loglik_per_tree,
    products: per non-root node n (columns [m], [k, m] object array of the exact products P_n[i, j] v_n[j]), for judging arg-max
    choices; None for the roots,
    bu_log10 [N, k] float: log10 of the exact max-product vectors (-inf for zeros),
    min_best_ratio (float): over the non-root nodes, the smallest row maximum of the node's products (an entry of its message) over
        the largest -- while it is far above the rounding of float64 the sweeps' clamp of negative P(t) dust cannot have acted on a
        maximum, and the relative tie test of choice_is_a_maximum is meaningful in every row).
    """
    parent, first_child, n_children = flat.parent, flat.first_child, flat.n_children
    N, k = np.asarray(masks).shape
    allowed = np.asarray(masks) != 0
    with decimal.localcontext(_CONTEXT):
        op = operator(spec, flat.dist, sf, tau, tf)
        pi = _dec_array(spec['pi'])
        v = [None] * N
        message = [None] * N
        products = [None] * N
        worst = None
        columns = {}
        for n in reversed(range(N)):
            row = np.array([ONE if a else ZERO for a in allowed[n]], dtype=object)
            fc = int(first_child[n])
            for c in range(fc, fc + int(n_children[n])):
                row = row * message[c]
            v[n] = row
            if parent[n] >= 0:
                nz = [j for j, x in enumerate(row) if x != 0]
                # (branches of the same length share the columns of P(t'): the spine of a caterpillar, the tips of a polytomy)
                key = (op.t[n], tuple(nz))
                if key not in columns:
                    columns[key] = op.pij_columns(n, nz)
                products[n] = (nz, columns[key] * row[nz][None, :])
                message[n] = products[n][1].max(axis=1)
                worst = _ratio(message[n], worst)
        per_tree = [_ln(max(pi * v[int(r)])) for r in flat.roots]
        bu_log10 = _log10_rows(v)
    return dict(loglik=sum(per_tree, ZERO), loglik_per_tree=per_tree, products=products, bu_log10=bu_log10,
                min_best_ratio=float(worst) if worst is not None else 1.0)


def scenario_log_probability(flat, masks, spec, sf, tau, tf, states):
    """
    ln of the probability of one assignment of states to all nodes (states [N]), per tree, as a list of Decimals:
    ln(pi[s_root] prod over the tree's non-root nodes n of P_n[s_parent(n), s_n]), P(t') built exactly row by row (pij_row);
    -Infinity for a tree in which a state is not allowed by its node's mask (or the product is not positive).  The largest value
    over all assignments is joint_pass's loglik_per_tree.
    """
    parent = flat.parent
    N = len(parent)
    allowed = np.asarray(masks) != 0
    states = [int(s) for s in np.asarray(states)]
    with decimal.localcontext(_CONTEXT):
        op = operator(spec, flat.dist, sf, tau, tf)
        pi = _dec_array(spec['pi'])
        tree_of = [0] * N   # the root of the node's tree
        total = {}
        rows = {}
        for n in range(N):   # parents first
            p = int(parent[n])
            s = states[n]
            tree_of[n] = n if p < 0 else tree_of[p]
            ok = 0 <= s < allowed.shape[1] and allowed[n, s]
            if p < 0:
                factor = pi[s] if ok else ZERO
            elif not ok:
                factor = ZERO
            else:
                key = (op.t[n], states[p])
                if key not in rows:
                    rows[key] = op.pij_row(n, states[p])
                factor = rows[key][s]
            r = tree_of[n]
            total[r] = factor if p < 0 else total[r] * factor
        return [_ln(total[int(r)]) for r in flat.roots]


def choice_is_a_maximum(products, n, i, j, rtol=Decimal('1e-12')):
    """Whether state j is an arg-max of row i of node n's exact products, up to products equal to rtol."""
    cols, prod = products[n]
    best = max(prod[i])
    if j not in cols:
        return best == 0
    with decimal.localcontext(_CONTEXT):
        return best - prod[i][cols.index(j)] <= rtol * best


def rel_error(value, exact):
    """|value - exact| / |exact| for a double against a Decimal, as a float."""
    with decimal.localcontext(_CONTEXT):
        return float(abs(Decimal(float(value)) - exact) / abs(exact))
