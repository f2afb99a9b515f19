"""
TEST INFRASTRUCTURE: the smallest forests whose level schedule has two-level and stacked units, with the columns (masks and
parameters) that tests/test_gpu_consumers_on_unit_schedules.py runs on them, and the consumers' references computed once per
process.  Host arithmetic only: tests/test_unit_schedule_cases_host.py holds every column listed here to a finite ln L and to
posterior rows that are not all zero, so that the GPU file skips nothing and filters no case out.

Forests (all with TUNE, the level schedule with units however small the forest):
    chained   synthetic.balanced_forest(7): 128 tips, 255 nodes; 16 two-level nodes and 5 stacked ones, both chains run
    clumps    optimiser_point_cases.forest('clumps'): 256 nodes, two trees, 46 zero-length branches; units, no chain
    ragged    test_gpu_parity._forest_with_balanced_clumps(40, seed=3): some three-child nodes; units, no chain
State counts: 17 and 20 (8 lanes x 4 with padding), 32 (8 x 4 full), 33 (16 x 4 bottom-up, 8 x 8 top-down, padded), 64 (8 x 8
bottom-up on the balanced forest, 16 x 4 elsewhere); all five on chained, 20 and 64 on the other two.

Columns: column c of a case has loglik_gradient_cases.masks(flat, k, c), which leaves the tips on zero-length branches
unobserved, frequencies(k, seed c) and rates(seed c, tau = TAUS[c % 2]); on chained the last four columns have the four kinds of
masks of test_gpu_td_chain.masks_of instead (observed, unobserved, ambiguous, restricted internal nodes).  Parameter set 1
("other parameters") moves every seed by 5 and swaps the two values of tau.
"""
import numpy as np

import expected_counts_ref as xref
import expected_history_ref as href
import history_time_ref as tref
import loglik_gradient_cases as cases
import loglik_gradient_ref as gref
import optimiser_point_cases
from oracle import pastml_oracle as orc
from pastml_amd import synthetic

BASE_TUNE = dict(BLOCK_NODES=0, SMALL_MANY_NODES=0, SUPER_MIN=1, STACK_MIN=1)   # (test_gpu_parity.LEVEL_SCHEDULE)
TUNE = dict(BASE_TUNE, SMALL_MAX_NODES=0)
TAUS = (0.0, 0.011)
KIND_F81 = 0

FOREST_KS = [('chained', 17), ('chained', 20), ('chained', 32), ('chained', 33), ('chained', 64),
             ('clumps', 20), ('clumps', 64), ('ragged', 20), ('ragged', 64)]
N_COLUMNS = dict(chained=5, clumps=5, ragged=2)
# (forest, k) whose columns are also run at parameter set 1: the call orders
OTHER_PARAMETERS = [('chained', 20), ('chained', 64), ('clumps', 64)]
USES = [(name, k, 0) for name, k in FOREST_KS] + [(name, k, 1) for name, k in OTHER_PARAMETERS]

_forests = {}


def forest(name):
    if name not in _forests:
        if name == 'chained':
            flat = synthetic.balanced_forest(7)
        elif name == 'clumps':
            flat = optimiser_point_cases.forest('clumps')[0]
        elif name == 'ragged':
            from test_gpu_parity import LEVEL_SCHEDULE, _forest_with_balanced_clumps
            assert LEVEL_SCHEDULE == BASE_TUNE
            flat = _forest_with_balanced_clumps(40, seed=3)
        else:
            raise ValueError(name)
        _forests[name] = flat
    return _forests[name]


_masks = {}


def masks(name, k):
    """int8 [columns, N, k]"""
    if (name, k) not in _masks:
        flat = forest(name)
        C = N_COLUMNS[name]
        out = np.stack([cases.masks(flat, k, c) for c in range(C)])
        if name == 'chained':
            from test_gpu_td_chain import masks_of
            internal = np.flatnonzero(flat.n_children > 0)
            for seed in range(7000 + k, 7100 + k):   # (one internal node in 50 of 127: the first seed that restricts two)
                out[C - 4:] = masks_of(flat, k, 4, np.random.default_rng(seed))
                if (out[C - 1, internal].sum(axis=1) < k).sum() >= 2:
                    break
            else:
                raise AssertionError('no seed restricts two internal nodes')
        out.setflags(write=False)
        _masks[name, k] = out
    return _masks[name, k]


def models(name, k, p=0):
    """[(spec, (sf, tau, tau_factor))] of parameter set p, one per column, as Engine.set_models takes them."""
    assert (name, k, p) in USES, (name, k, p)
    return [(dict(kind=KIND_F81, pi=cases.frequencies('F81', k, c + 5 * p)), cases.rates(c + 5 * p, TAUS[(c + p) % 2]))
            for c in range(N_COLUMNS[name])]


def node_times(name):
    return tref.root_distance(forest(name), stagger=0.21)


def boundaries(name):
    """Five bins: four that cut branches (one boundary exactly on a node), and one after the last tip, which is empty."""
    b = tref.covering_boundaries(node_times(name), 4)
    return np.concatenate((b, [b[-1] + 0.5]))


def altered(name):
    """0/1 [N]: the parents of the tips on zero-length branches (clumps); elsewhere the parents of every seventh tip."""
    flat = forest(name)
    tips = np.asarray(flat.tips)
    zero = tips[flat.dist[tips] == 0]
    out = np.zeros(flat.n_nodes, dtype=np.uint8)
    out[flat.parent[zero if len(zero) else tips[::7]]] = 1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the references, computed once per process whoever asks
# ---------------------------------------------------------------------------------------------------------------------

def _key(args, kwargs):
    out = []
    for a in list(args) + sorted(kwargs.items()):
        if hasattr(a, 'parent') and hasattr(a, 'dist'):
            a = (np.asarray(a.parent).tobytes(), np.asarray(a.dist).tobytes())
        elif isinstance(a, np.ndarray):
            a = (a.shape, a.dtype.str, a.tobytes())
        elif isinstance(a, dict):
            a = tuple((name, _key([value], {})) for name, value in sorted(a.items()))
        elif isinstance(a, (list, tuple)):
            a = _key(a, {})
        elif hasattr(a, '__name__'):
            a = a.__name__
        out.append(a)
    return tuple(out)


def once(function):
    """function, its results kept by the values of its arguments (a result is shared: nobody writes into it)."""
    kept = {}

    def call(*args, **kwargs):
        key = _key(args, kwargs)
        if key not in kept:
            kept[key] = function(*args, **kwargs)
        return kept[key]
    call.__name__ = function.__name__
    call.__doc__ = function.__doc__
    return call


gradient = once(gref.gradient)
history = once(href.history)
by_subdivision = once(tref.by_subdivision)
from_oracle = once(xref.from_oracle)
REFERENCES = [(gref, 'gradient', gradient), (href, 'history', history), (tref, 'by_subdivision', by_subdivision),
              (xref, 'from_oracle', from_oracle)]
