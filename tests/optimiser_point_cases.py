"""
TEST INFRASTRUCTURE: the column blocks an F81-family optimiser sends, built the way fit_parameters_steps builds them
(model -> two_point_scheme -> kernel_points), at the optimiser's own parameter values: the bounds and the start of the scaling
factor x the bounds and an inner value of tau.  Host arithmetic only: tests/test_f81_exact_ref.py holds the oracle to the
exact values on these inputs, tests/test_gpu_optimiser_points.py the device.
"""
import numpy as np

from pastml_amd import synthetic
from pastml_amd.annotation import ForestStats
from pastml_amd.batch import CharacterBatch, zero_clusters, one_hot_words, masks_from_words, two_point_scheme
from pastml_amd.models import PointBlock, KIND_F81
from pastml_amd.models.F81Model import F81Model
from pastml_amd.models.JCModel import JCModel
from pastml_amd.models.EFTModel import EFTModel
from pastml_amd.tree import FlatForest

N_TIPS, SEED = 120, 11
STATES = (2, 5, 20, 64, 130, 300)
# (k, family): free frequencies up to 20 states (k + 2 points per block), fixed ones beyond (3 points), one JC block
CASES = [(k, 'F81' if k <= 20 else 'EFT') for k in STATES] + [(5, 'JC')]
SF_TIMES_AVG = (0.001, 1., 10.)      # the bounds of sf and its start, in units of 1 / avg_nonzero_brlen
TAU_OVER_AVG = (0., 1e-3, 1.)        # the bounds of tau and a value inside, in units of avg_nonzero_brlen
SMOOTHING_POINTS = 4                 # [sf, tau, smoothing] and the base point: what a smoothing model's block holds

# a second, smaller forest whose shape gives the level schedule its two-level units (a node with two children that each carry two
# cherries of two tips) and stacked units: a random binary forest with half of its leaves replaced by balanced 8-tip subtrees
CLUMP_CASES = [(20, 'F81'), (64, 'EFT')]
CLUMP_LEAVES, CLUMP_SEED = 24, 5

_forest = {}


def clump_forest():
    """test_gpu_parity._forest_with_balanced_clumps in small, with a fifth of the branches set to zero length."""
    from pastml_amd.tree import TreeNode
    rng = np.random.default_rng(CLUMP_SEED)
    roots = []
    for _ in range(2):
        root = TreeNode(name='', dist=0.0)
        leaves = [root]
        while len(leaves) < CLUMP_LEAVES // 2:
            leaf = leaves.pop(int(rng.integers(len(leaves))))
            for _c in range(2):
                leaves.append(leaf.add_child(dist=float(rng.uniform(0.001, 0.3))))
        for leaf in leaves:
            if rng.random() < 0.5:
                level = [leaf]
                for _d in range(3):
                    level = [n.add_child(dist=0.0 if rng.random() < 0.2 else float(rng.uniform(0.001, 0.3)))
                             for n in level for _c in range(2)]
        roots.append(root)
    for ti, root in enumerate(roots):
        for i, n in enumerate(root.traverse('preorder')):
            n.name = 't{}_{}'.format(ti, i) if n.is_leaf() else 'n{}_{}'.format(ti, i)
    return FlatForest.from_trees(roots)


def forest(shape='random'):
    if shape not in _forest:
        flat = FlatForest.random(N_TIPS, SEED, max_arity=3, zero_frac=0.2, n_trees=2) if shape == 'random' else clump_forest()
        _forest[shape] = flat, ForestStats(flat)
    return _forest[shape]


def tip_words(flat, k, rng):
    """
    (words [2, N, W], annotated [2, N]) of two characters.  Character 0: every tip observed, and in every cluster of tips joined
    by zero-length branches the first two get different states -- the cases of the zero-branch alteration.  Character 1: the
    same states with 10 % of the tips missing and 10 % given two states.
    """
    N = flat.n_nodes
    tips = np.asarray(flat.tips)
    state = np.full(N, -1, dtype=np.int64)
    state[tips] = rng.integers(k, size=len(tips))
    zc = zero_clusters(flat)
    is_tip = np.zeros(N, dtype=bool)
    is_tip[tips] = True
    for a, b in zip(zc.starts, list(zc.starts[1:]) + [len(zc.nodes)]):
        members = [n for n in zc.nodes[a:b] if is_tip[n]]
        if len(members) >= 2 and state[members[0]] == state[members[1]]:
            state[members[1]] = (state[members[0]] + 1) % k
    words = np.zeros((2, N, (k + 63) // 64), dtype=np.uint64)
    words[0, tips] = one_hot_words(state[tips], k)
    words[1] = words[0]
    draw = rng.random(len(tips))
    words[1, tips[draw < 0.1]] = 0
    two = tips[(draw >= 0.1) & (draw < 0.2)]
    words[1, two] |= one_hot_words((state[two] + 1 + rng.integers(k - 1, size=len(two))) % k, k)
    return words, words.any(axis=-1)


def make_batch(flat, k, rng):
    batch = CharacterBatch(flat, k, 2)
    words, annotated = tip_words(flat, k, rng)
    for c in range(2):
        batch.set_annotation(c, words[c], annotated[c])
    batch.initialize_allowed_states()
    return batch


def altered_words(batch, c):
    """What CharacterBatch._altered_variant computes, without an optimiser context: the masks of character c after the zero-branch
    alteration, or None if it changes nothing.  The batch's masks are left as they were."""
    plain = batch.masks[c].copy()
    init, has = batch.init_masks[c].copy(), batch.has_init[c].copy()
    rows = np.zeros(batch.m, dtype=bool)
    rows[c] = True
    changed = batch.alter(rows)[c].any()
    words = batch.masks[c].copy() if changed else None
    batch.masks[c] = plain
    batch.init_masks[c], batch.has_init[c] = init, has
    return words


def make_model(family, k, stats, rng, smoothing=False):
    states = synthetic.state_names(k)
    pi = rng.dirichlet(np.ones(k) * 3)
    if smoothing:
        # as acr() builds it when the frequencies come in column2parameters: smoothed, not optimised
        return F81Model(states=states, forest_stats=stats, frequencies=pi, frequency_smoothing=True, optimise_tau=True)
    if family == 'JC':
        return JCModel(states=states, forest_stats=stats, optimise_tau=True)
    if family == 'EFT':
        return EFTModel(states=states, forest_stats=stats, observed_frequencies=pi, optimise_tau=True)
    return F81Model(states=states, forest_stats=stats, frequencies=pi, optimise_tau=True)


def base_points(stats):
    avg = stats.avg_nonzero_brlen
    return [(a / avg, b * avg) for a in SF_TIMES_AVG for b in TAU_OVER_AVG]


def block_at(model, sf, tau):
    """The points of one finite-difference gradient of ``model`` at (sf, tau) and its current frequencies: what
    search_parameters_steps.objective_and_gradient yields.  A PointBlock, or a list of (spec, rates) under frequency smoothing."""
    frequencies = np.array(model.frequencies)
    model._sf, model._tau = sf, tau
    model.calc_tau_factor()
    x0 = model.get_optimised_parameters()
    bounds = model.get_bounds()
    points, _ = two_point_scheme(x0, bounds[:, 0], bounds[:, 1])
    block = model.kernel_points(np.vstack((x0[None, :], points)))
    model._frequencies = frequencies
    return block


def as_arrays(block):
    """(pi [n, k], sf, tau, tf [n]) of a PointBlock or of a list of (spec, rates)."""
    if type(block) is PointBlock:
        return block.pi, block.sf, block.tau, block.tf
    rates = np.array([r for _, r in block], dtype=np.float64)
    return np.array([s['pi'] for s, _ in block], dtype=np.float64), rates[:, 0], rates[:, 1], rates[:, 2]


def as_point_block(block):
    pi, sf, tau, tf = as_arrays(block)
    return PointBlock(KIND_F81, np.ascontiguousarray(pi), sf.copy(), tau.copy(), tf.copy())


def column_masks(batch, c, tau, altered):
    """0/1 masks [N, k] of a column of character c: altered for a point with tau == 0 (where the alteration changes anything)."""
    words = batch.masks[c] if (tau != 0 or altered is None) else altered
    return masks_from_words(words, batch.k)


def regime(tau, avg):
    """'tiny' for the tau-step points next to 0, 'small' up to 1e-3 avg (+ a step), 'zero' and 'large' for the rest."""
    if tau == 0:
        return 'zero'
    if tau < 1e-6 * avg:
        return 'tiny'
    return 'small' if tau < 0.5 * avg else 'large'


_built = {}
_exact = {}


def build(k, family, shape='random'):
    """Everything of one case, built once per process: the forest, the batch (host side), a model and a smoothing model per
    character, the altered masks per character."""
    key = (k, family, shape)
    if key not in _built:
        flat, stats = forest(shape)
        rng = np.random.default_rng(1000 * k + len(family))
        batch = make_batch(flat, k, rng)
        _built[key] = dict(k=k, family=family, shape=shape, flat=flat, batch=batch, stats=stats,
                           models=[make_model(family, k, stats, rng) for _ in range(2)],
                           smoothing=[make_model(family, k, stats, rng, smoothing=True) for _ in range(2)],
                           altered=[altered_words(batch, c) for c in range(2)])
    return _built[key]


def width(b):
    return max(len(block_at(b['models'][0], *base_points(b['stats'])[0])), SMOOTHING_POINTS)


def all_blocks(b):
    """((character, sf, tau, 'staged' | 'tuples'), (pi, sf, tau, tf)) of every block of the case."""
    for sf0, tau0 in base_points(b['stats']):
        for c in range(2):
            yield (c, sf0, tau0, 'staged'), as_arrays(block_at(b['models'][c], sf0, tau0))
            yield (c, sf0, tau0, 'tuples'), as_arrays(block_at(b['smoothing'][c], sf0, tau0))


def exact_value(b, c, masks, pi, sf, tau, tf):
    """The exact bottom-up pass of one column (f81_exact_ref.marginal_pass), computed once per process."""
    import f81_exact_ref
    key = (b['k'], b['family'], b['shape'], c, masks.tobytes(), np.asarray(pi).tobytes(), float(sf), float(tau), float(tf))
    if key not in _exact:
        _exact[key] = f81_exact_ref.marginal_pass(b['flat'], masks, pi, sf, tau, tf)
    return _exact[key]
