"""
Maximum-likelihood ancestral character reconstruction: the host side of the hot path of ``pastml/ml.py``.

Same public functions, arguments, result dictionaries, node features and errors as the reference
(``ml_acr`` ml.py:640, ``get_bottom_up_loglikelihood`` :82, ``calculate_top_down_likelihood`` :240,
``calculate_marginal_likelihoods`` :431, ``convert_likelihoods_to_probabilities`` :486, ``optimise_likelihood`` :865,
``optimize_likelihood_params`` :174, the three ``choose_ancestral_states_*`` :505-622), but the tree is flattened once
into level-ordered arrays (:class:`ForestProblem`) and every likelihood sweep runs on the GPU through
``pastml_amd.hip.Engine`` (C-ABI ``include/pastml_hip.h``).  There is no CPU implementation of the sweeps in this
module: without the HIP library / an MI355X the calls raise.

What stays on the host, as SURVEY.md section 8a prescribes: the allowed-state masks and their zero-branch alteration
(ml.py:293-428), the scipy L-BFGS-B driver (:174-237), the per-node state selection rules (:505-595) and the
bookkeeping of results.
"""
import numpy as np
import pandas as pd

from pastml_amd import get_personalized_feature_name
from pastml_amd import hip
from pastml_amd.tree import TreeNode, get_flat_forest

LOG_LIKELIHOOD = 'log_likelihood'
RESTRICTED_LOG_LIKELIHOOD_FORMAT_STR = '{}_restricted_{{}}'.format(LOG_LIKELIHOOD)

JOINT = 'JOINT'
MPPA = 'MPPA'
MAP = 'MAP'
ALL = 'ALL'
ML = 'ML'

MARGINAL_PROBABILITIES = 'marginal_probabilities'

MODEL = 'model'

MIN_VALUE = np.log10(np.finfo(np.float64).eps)
MAX_VALUE = np.log10(np.finfo(np.float64).max)

MARGINAL_ML_METHODS = {MPPA, MAP}
ML_METHODS = MARGINAL_ML_METHODS | {JOINT}
META_ML_METHODS = {ML, ALL}

BU_LH = 'BOTTOM_UP_LIKELIHOOD'
TD_LH = 'TOP_DOWN_LIKELIHOOD'
LH = 'LIKELIHOOD'
LH_SF = 'LIKELIHOOD_SF'
BU_LH_SF = 'BOTTOM_UP_LIKELIHOOD_SF'
BU_LH_JOINT_STATES = 'BOTTOM_UP_LIKELIHOOD_JOINT_STATES'
TD_LH_SF = 'TOP_DOWM_LIKELIHOOD_SF'
ALLOWED_STATES = 'ALLOWED_STATES'
STATE_COUNTS = 'STATE_COUNTS'
JOINT_STATE = 'JOINT_STATE'


def is_marginal(method):
    """MAP, MPPA or one of the meta-methods (ALL, ML)."""
    return method in MARGINAL_ML_METHODS or method in META_ML_METHODS


def is_ml(method):
    """JOINT, a marginal method or a meta-method."""
    return method in ML_METHODS or method in META_ML_METHODS


def is_meta_ml(method):
    return method in META_ML_METHODS


def get_default_ml_method():
    return MPPA


class PastMLLikelihoodError(Exception):

    def __init__(self, *args):
        self.message = args[0] if args else None

    def __str__(self):
        if self.message:
            return 'PastMLLikelihoodError, {}'.format(self.message)
        return 'PastMLLikelihoodError has been raised.'


# =====================================================================================================================
# array-level problem: one character on one forest
# =====================================================================================================================

def zero_branch_tops(flat):
    """
    top[n] = the highest node reachable from n through zero-length branches (the representative of n's
    zero-distance cluster, ml.py:321-349).
    """
    from pastml_amd.batch import zero_clusters
    return zero_clusters(flat).top


class ForestProblem(object):
    """
    One character on one forest: a single-column view of :class:`pastml_amd.batch.CharacterBatch` (which holds the
    allowed-state masks of the reference's ``<character>_ALLOWED_STATES`` features as packed words, the masks saved by
    zero-branch alteration, and the device context) with the masks exposed as 0/1 arrays [N, k].  The stand-alone
    sweep functions of this module and ``marginal_counts`` work on it; ``ml_acr`` uses the batch directly.
    """

    def __init__(self, forest, character, states, flat=None, device=None):
        from pastml_amd.batch import CharacterBatch
        if isinstance(forest, TreeNode):
            forest = [forest]
        self.forest = forest
        self.character = character
        self.states = np.asarray(states)
        self.k = len(self.states)
        self.flat = flat if flat is not None else get_flat_forest(forest)
        self.nodes = self.flat.nodes
        self.N = self.flat.n_nodes
        self.batch = CharacterBatch(self.flat, self.k, 1, device=device)
        self._device = device
        self.pij_window_stats = None   # where the context finds P(t): planned before the first sweep (batch.consumer_window)

    # the reference's 0/1 arrays, converted on access
    @property
    def masks(self):
        return hip.unpack_masks(self.batch.masks[0], self.k)

    @masks.setter
    def masks(self, value):
        self.batch.masks[0] = hip.pack_masks(value, self.k)

    @property
    def init_masks(self):
        return hip.unpack_masks(self.batch.init_masks[0], self.k)

    @property
    def has_init(self):
        return self.batch.has_init[0]

    @property
    def annotated(self):
        return self.batch.annotated[0]

    @annotated.setter
    def annotated(self, value):
        self.batch.annotated[0] = value

    @property
    def n_sweeps(self):
        return self.batch.n_sweeps

    @property
    def engine(self):
        return self.batch.engine

    def close(self):
        self.batch.close()

    # ------------------------------------------------------------------------------------------------ masks
    def initialize_allowed_states(self):
        """Masks from the ``character`` feature of the nodes (ml.py:293-318), and which nodes "have a state"."""
        from pastml_amd.batch import annotation_words
        self.batch.set_annotation(0, *annotation_words(self.flat, self.character, self.states))
        self.batch.initialize_allowed_states()

    def alter_zero_node_allowed_states(self):
        """Zero-branch alteration (ml.py:352-387); returns the ids of the altered nodes."""
        return np.flatnonzero(self.batch.alter(np.ones(1, dtype=bool))[0])

    def unalter_zero_node_allowed_states(self, altered):
        """masks & saved masks, or the saved ones if nothing is left (ml.py:390-405)."""
        flags = np.zeros((1, self.N), dtype=bool)
        flags[0, np.asarray(altered, dtype=np.int64)] = True
        self.batch.unalter(flags)

    # ------------------------------------------------------------------------------------------------ device
    def bottom_up_loglikelihood(self, model, is_marginal=True, alter=True):
        """Sum over the trees of the forest of get_bottom_up_loglikelihood (ml.py:82-121)."""
        from pastml_amd.batch import LikelihoodError, consumer_window, likelihood_error
        if self.pij_window_stats is None:
            # a character whose whole-tree batch of P(t) does not fit the device runs with a window of it: the sweeps and what
            # marginal_counts / sample_scenarios do after them (MemoryError if not even the smallest window fits)
            self.batch.pij_window, self.pij_window_stats = consumer_window(
                self.flat, self.k, model.kernel_spec()['kind'], 1, self.character, 'ForestProblem', device=self._device)
        try:
            return float(self.batch.bottom_up([model], is_marginal=is_marginal, alter=alter)[0])
        except LikelihoodError as e:
            raise likelihood_error(self.flat, e)

    def select_on_device(self, method, force_joint=False):
        """MAP / MPPA selection (ml.py:505-595) on the device; returns the number of selected states per node."""
        return self.batch.select(method, force_joint=force_joint)[0]

    def joint_states(self):
        """Joint state of every node after a joint sweep (ml.py:598-622)."""
        return self.batch.joint_states()[0]

    def top_down_marginals(self):
        """
        After a marginal sweep: top-down sweep, marginal likelihoods and posteriors (ml.py:240-290, 431-502).
        Returns (posterior [N, k], lh [N, k], lh_sf [N]) where lh / lh_sf play the role of the reference's
        LIKELIHOOD / LIKELIHOOD_SF features: log10(lh.sum()) - lh_sf is the node's total log10-likelihood.
        """
        post, lh_sum, lh_sf = self.batch.top_down_marginals()
        return post[0], post[0] * lh_sum[0][:, None], lh_sf[0]

    def per_tree_order(self):
        """Node ids tree by tree, each in level order: the row order of the reference's probability table."""
        if len(self.flat.roots) == 1:
            return np.arange(self.N)
        return np.lexsort((np.arange(self.N), self.flat.tree_id))


# =====================================================================================================================
# state selection on arrays
# =====================================================================================================================

def select_map(lh):
    """One-hot masks at the arg-max of the marginal likelihoods (ml.py:591-595)."""
    N, k = lh.shape
    masks = np.zeros((N, k), dtype=np.int8)
    masks[np.arange(N), lh.argmax(axis=1)] = 1
    return masks


def select_mppa(lh, joint_state=None, chunk=1 << 16):
    """
    Marginal posterior probabilities approximation (ml.py:539-572) for all nodes at once.
    lh: [N, k] marginal likelihoods (already multiplied by the saved masks where the reference does so);
    joint_state: [N] to force the joint state into the selection (force_joint), or None.
    Returns (masks [N, k] int8, best_k [N]).

    Per node: the probabilities are sorted ascending (the joint state's one is moved last), the number m of kept
    states minimises sum((0,..,0,1/m,..,1/m) - sorted)^2 (first minimum), and the m states with the largest
    likelihoods are kept (stable order, i.e. ties go to the lower index -- the reference's sort key has a constant
    first component, ml.py:562-563).
    """
    N, k = lh.shape
    masks = np.zeros((N, k), dtype=np.int8)
    best_ks = np.zeros(N, dtype=np.int64)
    for a in range(0, N, chunk):
        b = min(N, a + chunk)
        ml = lh[a:b]
        probs = ml / ml.sum(axis=1)[:, None]
        if joint_state is not None:
            ji = joint_state[a:b]
            rows = np.arange(b - a)
            jp = probs[rows, ji]
            rest = probs.copy()
            rest[rows, ji] = np.inf  # sorts last, then replaced by the joint probability
            q = np.sort(rest, axis=1)
            q[:, -1] = jp
        else:
            q = np.sort(probs, axis=1)
        best_c = np.full(b - a, np.inf)
        best_k = np.full(b - a, k, dtype=np.int64)
        for m in range(1, k + 1):
            u = np.hstack((np.zeros(k - m), np.ones(m) / m))
            corr = u[None, :] - q
            corr = (corr * corr).sum(axis=1)
            better = corr < best_c
            best_c[better] = corr[better]
            best_k[better] = m
        order = np.argsort(-ml, axis=1, kind='stable')
        keep = np.arange(k)[None, :] < best_k[:, None]
        sel = np.zeros((b - a, k), dtype=np.int8)
        np.put_along_axis(sel, order, keep.astype(np.int8), axis=1)
        masks[a:b] = sel
        best_ks[a:b] = best_k
    return masks, best_ks


# =====================================================================================================================
# reference-shaped functions on trees
# =====================================================================================================================

def _problem_of(tree, character, model):
    """The ForestProblem cached on a tree for the stand-alone API functions."""
    cache = tree.__dict__.setdefault('_pastml_amd_problems', {})
    flat = get_flat_forest([tree])
    problem = cache.get(character)
    if problem is None or problem.flat is not flat or problem.k != len(model.states):
        if problem is not None:
            problem.close()
        problem = ForestProblem([tree], character, model.states, flat=flat)
        cache[character] = problem
    return problem


def initialize_allowed_states(tree, feature, states):
    """Adds the ``<feature>_ALLOWED_STATES`` arrays to the nodes (ml.py:293-318)."""
    allowed_states_feature = get_personalized_feature_name(feature, ALLOWED_STATES)
    n = len(states)
    state2index = dict(zip(states, range(n)))
    for node in tree.traverse():
        node_states = getattr(node, feature, set())
        if not node_states:
            allowed_states = np.ones(n, dtype=int)
        else:
            allowed_states = np.zeros(n, dtype=int)
            for state in node_states:
                allowed_states[state2index[state]] = 1
        node.add_feature(allowed_states_feature, allowed_states)


def _pull_masks_from_features(problem, tree, character):
    """Reads the node features into the problem's arrays (stand-alone API path)."""
    A = get_personalized_feature_name(character, ALLOWED_STATES)
    init = A + '.initial'
    N, k = problem.N, problem.k
    masks = np.zeros((N, k), dtype=np.int8)
    saved = np.zeros((N, k), dtype=np.int8)
    for i, node in enumerate(problem.nodes):
        masks[i] = getattr(node, A)
        value = getattr(node, character, None)
        problem.batch.annotated[0, i] = value is not None and value != ''
        if hasattr(node, init):
            problem.batch.has_init[0, i] = True
            saved[i] = getattr(node, init)
    problem.masks = masks
    problem.batch.init_masks[0] = hip.pack_masks(saved, k)


def _push_masks_to_features(problem, character):
    A = get_personalized_feature_name(character, ALLOWED_STATES)
    init = A + '.initial'
    masks, saved, has = problem.masks, problem.init_masks, problem.has_init
    for i, node in enumerate(problem.nodes):
        node.add_feature(A, masks[i].astype(int))
        if has[i]:
            node.add_feature(init, saved[i].astype(int))


def get_bottom_up_loglikelihood(tree, character, model, is_marginal=True, alter=True):
    """
    Bottom-up log-likelihood of one tree for the masks stored in the ``<character>_ALLOWED_STATES`` node features
    (API of ml.py:82-121).  The per-node vectors stay on the device; ``<character>_BOTTOM_UP_LIKELIHOOD`` and
    ``..._SF`` features are written back so that callers that read them keep working.
    """
    problem = _problem_of(tree, character, model)
    _pull_masks_from_features(problem, tree, character)
    res = problem.bottom_up_loglikelihood(model, is_marginal=is_marginal, alter=alter)
    _push_masks_to_features(problem, character)
    bu = problem.engine.download(hip.BUF_BU)
    bu_sf = problem.engine.download(hip.BUF_BU_SF)
    lh_feature = get_personalized_feature_name(character, BU_LH)
    lh_sf_feature = get_personalized_feature_name(character, BU_LH_SF)
    for i, node in enumerate(problem.nodes):
        node.add_feature(lh_feature, bu[i])
        node.add_feature(lh_sf_feature, bu_sf[i])
    if not is_marginal:
        table = problem.engine.download(hip.BUF_JOINT_TABLE).astype(np.int64)
        f = get_personalized_feature_name(character, BU_LH_JOINT_STATES)
        for i, node in enumerate(problem.nodes):
            if not node.is_root():
                node.add_feature(f, table[i])
    return res


def calculate_top_down_likelihood(tree, character, model):
    """
    Top-down likelihoods (API of ml.py:240-270); must follow a marginal get_bottom_up_loglikelihood on the same tree.
    The device computes the top-down vectors, the marginal likelihoods and the posteriors in one fused sweep.
    """
    problem = _problem_of(tree, character, model)
    post, lh, lh_sf = problem.top_down_marginals()
    problem.last_marginals = (post, lh, lh_sf)
    td = problem.engine.download(hip.BUF_TD)
    td_sf = problem.engine.download(hip.BUF_TD_SF)
    f, fsf = get_personalized_feature_name(character, TD_LH), get_personalized_feature_name(character, TD_LH_SF)
    for i, node in enumerate(problem.nodes):
        node.add_feature(f, td[i])
        node.add_feature(fsf, td_sf[i])


def calculate_marginal_likelihoods(tree, feature, frequencies, clean_up=True):
    """
    Stores ``<feature>_LIKELIHOOD`` / ``_LIKELIHOOD_SF`` on the nodes (API of ml.py:431-465) from the fused device
    sweep run by calculate_top_down_likelihood.
    """
    problem = tree.__dict__.get('_pastml_amd_problems', {}).get(feature)
    if problem is None or getattr(problem, 'last_marginals', None) is None:
        raise ValueError('calculate_top_down_likelihood must be called first')
    post, lh, lh_sf = problem.last_marginals
    lh_feature = get_personalized_feature_name(feature, LH)
    lh_sf_feature = get_personalized_feature_name(feature, LH_SF)
    for i, node in enumerate(problem.nodes):
        node.add_feature(lh_feature, lh[i].copy())
        node.add_feature(lh_sf_feature, lh_sf[i])
        if clean_up:
            for name in (BU_LH, BU_LH_SF, TD_LH, TD_LH_SF):
                node.del_feature(get_personalized_feature_name(feature, name))


def convert_likelihoods_to_probabilities(tree, feature, states):
    """DataFrame node name -> marginal probabilities, rows in tree.traverse() order (ml.py:486-502)."""
    lh_feature = get_personalized_feature_name(feature, LH)
    names, rows = [], []
    for node in tree.traverse():
        lh = getattr(node, lh_feature)
        names.append(node.name)
        rows.append(lh / lh.sum())
    return pd.DataFrame(np.array(rows), index=names, columns=states)


def convert_allowed_states2feature(tree, feature, states, out_feature=None):
    if out_feature is None:
        out_feature = feature
    allowed_states_feature = get_personalized_feature_name(feature, ALLOWED_STATES)
    for node in tree.traverse():
        node.add_feature(out_feature, set(states[getattr(node, allowed_states_feature).astype(bool)]))


# =====================================================================================================================
# parameter optimisation (API of ml.py:174-237, 865-920; the procedure itself lives in pastml_amd.batch)
# =====================================================================================================================

def _single_character_evaluator(problem):
    """evaluate(points) for the optimiser of one character: a bottom-up sweep with one column per point."""
    from pastml_amd.batch import LikelihoodError, likelihood_error
    batch = problem.batch

    def evaluate(points):
        out = batch.evaluate_points({0: points})[0]
        if isinstance(out, LikelihoodError):
            raise likelihood_error(problem.flat, out)
        return out
    return evaluate


def optimize_likelihood_params(forest, character, observed_frequencies, model, problem=None):
    """
    L-BFGS-B over the model's currently free parameters (API of ml.py:174-237); every function evaluation -- every
    whole finite-difference gradient -- is one bottom-up sweep on the GPU.  The model is left at the optimum.
    """
    from pastml_amd.batch import search_parameters, block_width
    own = problem is None
    if own:
        problem = ForestProblem(forest, character, model.states)
        problem.initialize_allowed_states()
    try:
        opened = problem.batch._opt is None
        if opened:
            problem.batch.open_optimiser([block_width(model)])
        evaluate = _single_character_evaluator(problem)

        def evaluate_vectors(vectors):
            points = []
            for ps in vectors:
                model.set_params_from_optimised(ps)
                points.append((model.kernel_spec(), model.rate_params()))
            return evaluate(points)
        try:
            return search_parameters(model, observed_frequencies, evaluate_vectors,
                                     np.random.RandomState(np.random.randint(0, 2 ** 31 - 1)))
        finally:
            if opened:
                hip.release_engine(problem.batch._opt['engine'])
                problem.batch._opt = None
    finally:
        if own:
            problem.close()


def optimise_likelihood(forest, character, model, observed_frequencies, problem=None):
    """Initial likelihood, then the scaling / smoothing factors, then all free parameters (API of ml.py:865-920)."""
    from pastml_amd.batch import fit_parameters, block_width
    own = problem is None
    if own:
        problem = ForestProblem(forest, character, model.states)
    try:
        problem.initialize_allowed_states()
        problem.batch.open_optimiser([block_width(model)])
        try:
            return fit_parameters(character, model, observed_frequencies, _single_character_evaluator(problem),
                                  np.random.RandomState(np.random.randint(0, 2 ** 31 - 1)))
        finally:
            hip.release_engine(problem.batch._opt['engine'])
            problem.batch._opt = None
    finally:
        if own:
            problem.close()


# =====================================================================================================================
# ml_acr
# =====================================================================================================================

def ml_acr(forest, character, prediction_method, model, observed_frequencies, force_joint=True):
    """
    ML states on the trees, stored in node features; returns the list of result dictionaries (ml.py:640-750).

    Node features written (as the reference leaves them, here as columnar features of the flattened forest):
    ``<character>`` (set of selected states), ``<character>_ALLOWED_STATES``, ``<character>_JOINT_STATE`` (unless
    MAP), ``<character>_LIKELIHOOD`` / ``_LIKELIHOOD_SF`` (marginal methods).  One character is a batch of one:
    ``pastml_amd.acr.acr`` hands all characters of a run to :func:`pastml_amd.batch.run_tasks` together.
    """
    from pastml_amd.batch import Task, run_tasks
    return run_tasks(forest, [Task(character, prediction_method, model, observed_frequencies)],
                     force_joint=force_joint)[0]


# =====================================================================================================================
# marginal_counts
# =====================================================================================================================

def marginal_counts(forest, character, model, n_repetitions=1_000, device_sampling=True):
    """
    Expected numbers of state changes i -> j along the trees, estimated by drawing ``n_repetitions`` ancestral
    scenarios from the marginal posterior (API and sampling scheme of pastml/ml.py:753-862, used by
    utilities/transition_counter.py).

    The likelihood part -- bottom-up and top-down sweeps, root posteriors, per-branch P(t) -- runs on the GPU, and so
    does the scenario sampling (draws of child states given the parent's state counts, ml.py:818-857:
    ``pml_marginal_counts``).  Where zero-branch handling altered some nodes the draws are still the device's
    (``pml_marginal_counts_altered``); the fractional counts the reference gives the (parent, child) pairs with an altered end
    (ml.py:806-812, 840-853) are formed here from the nodes' state counts.  More than 256 states, or
    ``device_sampling=False``: the host sampler with numpy's generator, line by line the reference's.  Either way only
    statistical parity with the reference is meaningful.

    :param device_sampling: False forces the host sampler (tests compare the two)
    :return: k x k array, entry [i, j] = average number of i -> j changes per scenario
    """
    if isinstance(forest, TreeNode):
        forest = [forest]
    problem = ForestProblem(forest, character, model.states)
    try:
        k = problem.k
        flat = problem.flat
        problem.initialize_allowed_states()
        altered = problem.alter_zero_node_allowed_states() if 0 == model.tau else np.zeros(0, dtype=np.int64)
        problem.bottom_up_loglikelihood(model, is_marginal=True, alter=False)
        marginal_counts.last_stats = dict(pij_window=[problem.pij_window_stats])
        posterior, _, _ = problem.top_down_marginals()
        if device_sampling and not len(altered) and k <= 256:   # (the device sampler's tables hold 256 states)
            # no node altered by the zero-branch handling: the scenarios are drawn on the device (same scheme, a
            # counter-based generator seeded from numpy's global one, so np.random.seed still fixes the result)
            return problem.engine.marginal_counts(n_repetitions, seed=int(np.random.randint(0, 2 ** 62, dtype=np.int64)))
        if device_sampling and k <= 256:
            # altered nodes: the draws are the device's all the same; the pairs with an altered end get their fractional counts
            # here (ml.py:806-812, 840-853), from the nodes' state counts, and their parents the diagonal correction (:857-858)
            is_altered = np.zeros(problem.N, dtype=bool)
            is_altered[altered] = True
            sums, counts, same_int = problem.engine.marginal_counts_altered(
                n_repetitions, int(np.random.randint(0, 2 ** 62, dtype=np.int64)), is_altered)
            initial = problem.init_masks

            def to_initial(cnt, n):
                c = cnt * initial[n]
                if np.count_nonzero(c):
                    return n_repetitions * c / c.sum()
                return n_repetitions * initial[n].astype(np.float64) / initial[n].sum()   # (int8 masks: the product must not be formed in int8)

            result = sums
            internal = np.flatnonzero(flat.n_children > 0)
            fcs, ncs = flat.first_child, flat.n_children
            has_altered_child = np.zeros(problem.N, dtype=bool)
            has_altered_child[flat.parent[altered][flat.parent[altered] >= 0]] = True
            for parent in internal[is_altered[internal] | has_altered_child[internal]]:
                pcounts = counts[parent].astype(np.float64)
                ps = to_initial(pcounts, parent) if is_altered[parent] else pcounts
                same = same_int[parent].astype(np.float64)
                pos = ps > 0
                for node in range(fcs[parent], fcs[parent] + ncs[parent]):
                    if not (is_altered[parent] or is_altered[node]):
                        continue
                    ccounts = counts[node].astype(np.float64)
                    ci = to_initial(ccounts, node) if is_altered[node] else ccounts
                    norm = ci / ci.sum()
                    result[pos] += ps[pos, None] * norm[None, :]
                    same[pos] += ps[pos] * norm[pos]
                result[np.arange(k), np.arange(k)] -= np.minimum(ps, same)
            return result / n_repetitions
        bu = problem.engine.download(hip.BUF_BU)
        # (an eigen model's P(0) carries +-1e-17 where the exact value is 0: clamped, as the device sampler and the sweeps do)
        P = np.maximum(problem.engine.pij_batch(copy_out=True)[0], 0.0)
        frequencies = np.asarray(model.frequencies, dtype=np.float64)
        is_altered = np.zeros(problem.N, dtype=bool)
        is_altered[altered] = True
        masks = problem.masks
        initial = problem.init_masks

        def restrict_to_initial(counts, n):
            """ml.py:806-812 / 840-846: counts of an altered node projected on its own (unaltered) states."""
            c = counts * initial[n]
            if np.count_nonzero(c):
                return n_repetitions * c / c.sum()
            return n_repetitions * initial[n].astype(np.float64) / initial[n].sum()   # (int8 masks: the product must not be formed in int8)

        result = np.zeros((k, k), dtype=float)
        state_counts = np.zeros((problem.N, k), dtype=np.int64)
        for parent in range(problem.N):
            if flat.parent[parent] < 0:
                state_counts[parent] = np.random.multinomial(n_repetitions, posterior[parent] / posterior[parent].sum())
            nc = flat.n_children[parent]
            if nc == 0:
                continue
            parent_counts = state_counts[parent]
            ps_counts_initial = restrict_to_initial(parent_counts, parent) if is_altered[parent] else parent_counts
            same_state_counts = np.zeros(k)
            fc = flat.first_child[parent]
            for node in range(fc, fc + nc):
                # p(child = b | parent = a)  ~  BU_node[b] * P[b, a] * pi_b * mask_b   (ml.py:819-824)
                weights = (bu[node] * frequencies * masks[node])[None, :] * P[node].T
                with np.errstate(divide='ignore', invalid='ignore'):  # rows of impossible parent states are unused
                    probs = weights / weights.sum(axis=1)[:, None]
                update_results = not is_altered[parent] and not is_altered[node]
                counts = np.zeros(k, dtype=np.int64)
                for j in np.flatnonzero(parent_counts):
                    drawn = np.random.multinomial(parent_counts[j], probs[j])
                    counts += drawn
                    if update_results:
                        result[j, :] += drawn
                        same_state_counts[j] += drawn[j]
                if not update_results:
                    counts_initial = restrict_to_initial(counts, node) if is_altered[node] else counts
                    norm_counts = counts_initial / counts_initial.sum()
                    for i in np.flatnonzero(ps_counts_initial > 0):
                        adjusted = norm_counts * ps_counts_initial[i]
                        result[i, :] += adjusted
                        same_state_counts[i] += adjusted[i]
                state_counts[node] = counts
            for i in range(k):
                result[i, i] -= min(ps_counts_initial[i], same_state_counts[i])
        return result / n_repetitions
    finally:
        problem.close()


# =====================================================================================================================
# expected_counts
# =====================================================================================================================

def add_altered_pairs(flat, counts, same, posterior, is_altered, initial):
    """
    The host part of expected_counts for one character with nodes altered by the zero-branch handling: the (parent, child)
    pairs with an altered end (pastml/ml.py:806-812, 840-855) and the diagonal correction of their parents (:859-860), for
    all affected parents at once.

    :param counts: [k, k] the device's sums over all other pairs (diagonal corrected for all other parents)
    :param same: [N, k] the affected parents' same-state sums over their other children (pml_expected_counts' same_out)
    :param posterior: [N, k] marginal posteriors = the per-scenario state frequencies q of the nodes
    :param is_altered: [N] bool; initial: [N, k] 0/1 masks the altered nodes had before
    :return: [k, k]
    """
    result = np.array(counts, dtype=np.float64)
    parent = flat.parent
    has_parent = parent >= 0
    child = np.flatnonzero(has_parent & (is_altered | is_altered[np.where(has_parent, parent, 0)]))
    if not len(child):
        return result
    par = parent[child]

    def states_of(nodes):
        # to_initial(q, x) for the altered nodes: q restricted to the states x had and renormalised, or those states evenly
        q = posterior[nodes]
        init = initial[nodes].astype(np.float64)
        c = q * init
        s = c.sum(axis=1, keepdims=True)
        restricted = np.where(s > 0, c / np.where(s > 0, s, 1.0), init / np.maximum(init.sum(axis=1, keepdims=True), 1.0))
        return np.where(is_altered[nodes][:, None], restricted, q)

    ps = states_of(par)
    ci = states_of(child)
    norm = ci / ci.sum(axis=1, keepdims=True)
    result += ps.T.dot(norm)   # (rows i with ps[i] == 0 add nothing, ml.py:851)
    same = np.array(same, dtype=np.float64)
    np.add.at(same, par, ps * norm)
    dirty = np.unique(par)
    result[np.diag_indices_from(result)] -= np.minimum(states_of(dirty), same[dirty]).sum(axis=0)
    return result


def expected_counts(forest, characters, models):
    """
    Exact expected numbers of state changes i -> j along the trees, per scenario: what marginal_counts (pastml/ml.py:753-862)
    estimates, in closed form -- its limit for n_repetitions -> infinity, term by term, diagonal correction and the fractional
    counts around altered nodes included; nothing is sampled.

    The quantity, for one character, nodes in level order.  M_n[a][b] is the reference's conditional (ml.py:819-824):
    w_n[b] = BU_n[b] * pi_b * mask_n[b], M_n[a][b] = w_n[b] * P_n[b][a] / sum_b' w_n[b'] * P_n[b'][a]; rows a with
    q_parent[a] == 0 are never used (ml.py:831).  Masks are the ones the marginal pass ran with (altered where tau == 0).
    q_root = marginal posterior of the root (ml.py:794-798), q_n = q_parent . M_n for every other node (the models are
    reversible, so q_n is the marginal posterior of n and is read from the posterior table).  A pair (p, n) with neither end
    altered adds q_p[a] * M_n[a][b] to result[a][b] and q_p[a] * M_n[a][a] to same_p[a].  A pair with an altered end
    (ml.py:806-812, 840-855): ps = to_initial(q_p, p) if p is altered else q_p, ci likewise for n, norm = ci / sum(ci); for
    every i with ps[i] > 0 result[i][:] += norm * ps[i], same_p[i] += norm[i] * ps[i]; to_initial(q, x) = q * initial_mask_x
    renormalised, or initial_mask_x / its sum if that product is all zero.  After the children of p (ml.py:859-860):
    result[i][i] -= min(ps[i], same_p[i]).

    Characters are grouped by (number of states, model kind); a group is one batch on the device: one marginal pass and
    ``pml_expected_counts`` over its columns (HIP, all characters at once; include/pastml_hip.h), the pairs around altered
    nodes are added here from posterior rows.  F81 family: up to 512 states; HKY and the eigen models: up to 256.

    :param characters: a character (feature name) or a list of them; models: a model or a list, one per character
    :return: a k x k array, entry [i, j] = expected number of i -> j changes per scenario -- or a list of them
    """
    from pastml_amd.batch import CharacterBatch, LikelihoodError, annotation_words, consumer_window, likelihood_error
    if isinstance(forest, TreeNode):
        forest = [forest]
    expected_counts.last_stats = dict(pij_window=[])   # per group: where its context finds P(t) (batch.consumer_window)
    single = isinstance(characters, str)
    if single:
        characters, models = [characters], [models]
    characters, models = list(characters), list(models)
    if len(characters) != len(models):
        raise ValueError('one model per character expected')
    flat = get_flat_forest(forest)
    groups = {}
    for i, model in enumerate(models):
        groups.setdefault((len(model.states), model.kernel_spec()['kind']), []).append(i)
    results = [None] * len(characters)
    for (k, kind), members in groups.items():
        group_models = [models[i] for i in members]
        window, record = consumer_window(flat, k, kind, len(members), characters[members[0]], 'expected_counts')
        expected_counts.last_stats['pij_window'].append(record)
        with CharacterBatch(flat, k, len(members)) as batch:
            batch.pij_window = window
            for c, i in enumerate(members):
                batch.set_annotation(c, *annotation_words(flat, characters[i], models[i].states))
            batch.initialize_allowed_states()
            try:
                altered = batch.marginal_pass_resident(group_models)
            except LikelihoodError as e:
                raise likelihood_error(flat, e)
            eng = batch.engine
            dirty = altered.any(axis=1)
            c = 0
            while c < len(members):
                if dirty[c]:
                    counts, same = eng.expected_counts(c, c + 1, altered=altered[c])
                    results[members[c]] = add_altered_pairs(flat, counts[0], same[0], eng.download(hip.BUF_POSTERIOR, c),
                                                            altered[c], hip.unpack_masks(batch.init_masks[c], k))
                    c += 1
                    continue
                e = c
                while e < len(members) and not dirty[e]:
                    e += 1
                for j, counts in enumerate(eng.expected_counts(c, e)):
                    results[members[c + j]] = counts
                c = e
    return results[0] if single else results


# =====================================================================================================================
# loglikelihood_gradient
# =====================================================================================================================

def loglikelihood_gradient(forest, characters, models):
    """
    Exact gradient of the marginal log-likelihood ln L of one character or a list of them under F81-family models (F81, JC,
    EFT): what ``get_bottom_up_loglikelihood(..., is_marginal=True, alter=True)`` evaluates, differentiated in closed form --
    no finite differences.  The likelihood is multilinear in the per-branch matrices, so the gradient is one streaming pass
    (``pml_loglik_gradient``, HIP; include/pastml_hip.h has the sums) over the vectors a marginal pass leaves on the device.

    Characters are grouped by their number of states; a group is one batch on the device: one marginal pass (masks altered
    where tau == 0, restored afterwards) and one gradient pass over its columns.

    :param characters: a character (feature name) or a list of them; models: a model or a list, one per character
    :return: per character a dict with ``log_likelihood``; the natural derivatives ``sf``, ``tau`` (total: through the branch
        transform and its tau factor) and ``frequencies`` ([k], every frequency treated as free, the dependence of mu on them
        included); ``parameters``: the gradient with respect to ``model.get_optimised_parameters()``, in its order (None for a
        model with frequency smoothing, whose chain rule is not implemented), with ``parameter_names``; and
        ``n_zero_length_branches``: the branches with exp(-mu t') == 1.  Where that count is not zero, ``tau`` (and its entry
        of ``parameters``) is NaN: such a branch leaves no trace of its share in the stored posteriors.
    """
    from pastml_amd import sharding
    from pastml_amd.batch import CharacterBatch, LikelihoodError, annotation_words, likelihood_error
    from pastml_amd.models import KIND_F81
    if isinstance(forest, TreeNode):
        forest = [forest]
    single = isinstance(characters, str)
    if single:
        characters, models = [characters], [models]
    characters, models = list(characters), list(models)
    if len(characters) != len(models):
        raise ValueError('one model per character expected')
    for character, model in zip(characters, models):
        if model.kernel_spec()['kind'] != KIND_F81:
            raise NotImplementedError('Character {}: loglikelihood_gradient is for the F81 family (F81, JC, EFT), not for {} '
                                      '(PML_ERR_UNSUPPORTED).'.format(character, getattr(model, 'name', type(model).__name__)))
    world = sharding.rank_world()[1]
    if world > 1:
        raise NotImplementedError('loglikelihood_gradient is not supported under a multi-process launch ({} ranks): run it in '
                                  'a single process'.format(world))
    flat = get_flat_forest(forest)
    groups = {}
    for i, model in enumerate(models):
        groups.setdefault(len(model.states), []).append(i)
    results = [None] * len(characters)
    for k, members in groups.items():
        group_models = [models[i] for i in members]
        with CharacterBatch(flat, k, len(members)) as batch:
            for c, i in enumerate(members):
                batch.set_annotation(c, *annotation_words(flat, characters[i], models[i].states))
            batch.initialize_allowed_states()
            try:
                lnl, d_rates, d_pi, n_flat = batch.loglik_gradient(group_models)
            except LikelihoodError as e:
                raise likelihood_error(flat, e)
        for c, i in enumerate(members):
            model = models[i]
            flat_branches = int(n_flat[c])
            tau = model.loglik_gradient_tau(d_rates[c], flat_branches)
            parameters, names = None, None
            if not model.frequency_smoothing_is_free():   # (the one case whose chain rule is refused)
                parameters, names = model.loglik_gradient_parameters(d_rates[c], d_pi[c], flat_branches), \
                    model.optimised_parameter_names()
            results[i] = dict(log_likelihood=float(lnl[c]), sf=float(d_rates[c, 0]), tau=float(tau), frequencies=d_pi[c].copy(),
                              parameters=parameters, parameter_names=names, n_zero_length_branches=flat_branches)
    return results[0] if single else results


# =====================================================================================================================
# expected_history
# =====================================================================================================================

def expected_history(forest, characters, models, branch_jumps=False):
    """
    Exact expected dwell times and numbers of Markov jumps along the trees, under the posterior over whole histories, of one
    character or a list of them under F81-family models (F81, JC, EFT): what stochastic mapping estimates by sampling, in closed
    form (``pml_expected_history``, HIP; include/pastml_hip.h has the sums) from the vectors a marginal pass leaves on the device.

    ``expected_counts`` compares the two ends of each branch and applies PastML's diagonal rule: it counts end-point
    differences.  This counts events -- a change that is undone on the same branch is two jumps here and nothing there -- and says
    how long the lineages spent in each state, which turns a count into a rate.

    Characters are grouped by their number of states; a group is one batch on the device: one marginal pass (masks altered
    where tau == 0, restored afterwards) and one pass over its columns.  HKY and the eigen models, the file-level front end and
    sharding over ranks are not covered.

    :param characters: a character (feature name) or a list of them; models: a model or a list, one per character
    :param branch_jumps: also return the expected number of jumps on the branch above every node
    :return: per character a dict with ``log_likelihood``; ``states``; ``times`` [k]: the expected time spent in each state, in
        units of smoothed branch length ((dist + tau) * tau_factor), summing to ``tree_length``, the sum of those lengths;
        ``jumps`` [k, k]: entry [i, j] = expected number of jumps i -> j, zero diagonal; and, when asked for, ``branch_jumps``
        [N] in FlatForest node order (0 for a root).
    """
    from pastml_amd import sharding
    from pastml_amd.batch import CharacterBatch, LikelihoodError, annotation_words, likelihood_error
    from pastml_amd.models import KIND_F81
    if isinstance(forest, TreeNode):
        forest = [forest]
    single = isinstance(characters, str)
    if single:
        characters, models = [characters], [models]
    characters, models = list(characters), list(models)
    if len(characters) != len(models):
        raise ValueError('one model per character expected')
    for character, model in zip(characters, models):
        if model.kernel_spec()['kind'] != KIND_F81:
            raise NotImplementedError('Character {}: expected_history is for the F81 family (F81, JC, EFT), not for {} '
                                      '(PML_ERR_UNSUPPORTED).'.format(character, getattr(model, 'name', type(model).__name__)))
    world = sharding.rank_world()[1]
    if world > 1:
        raise NotImplementedError('expected_history is not supported under a multi-process launch ({} ranks): run it in '
                                  'a single process'.format(world))
    flat = get_flat_forest(forest)
    groups = {}
    for i, model in enumerate(models):
        groups.setdefault(len(model.states), []).append(i)
    results = [None] * len(characters)
    has_parent = flat.parent >= 0
    for k, members in groups.items():
        group_models = [models[i] for i in members]
        with CharacterBatch(flat, k, len(members)) as batch:
            for c, i in enumerate(members):
                batch.set_annotation(c, *annotation_words(flat, characters[i], models[i].states))
            batch.initialize_allowed_states()
            try:
                lnl, times, jumps, per_branch = batch.expected_history(group_models, jumps=True, branch_jumps=branch_jumps)
            except LikelihoodError as e:
                raise likelihood_error(flat, e)
        for c, i in enumerate(members):
            _, tau, tau_factor = models[i].rate_params()
            result = dict(log_likelihood=float(lnl[c]), states=np.array(models[i].states), times=times[c].copy(),
                          jumps=jumps[c].copy(), tree_length=float(((flat.dist[has_parent] + tau) * tau_factor).sum()))
            if branch_jumps:
                result['branch_jumps'] = per_branch[c].copy()
            results[i] = result
    return results[0] if single else results


class _AsEigenModel(object):
    """An HKY model as the batch sees an eigen model: everything is the model's but the kernel description."""

    def __init__(self, model):
        self._model = model

    def __getattr__(self, name):
        return getattr(self._model, name)

    def kernel_spec(self):
        return self._model.eigen_spec()


def expected_history_general(forest, characters, models, branch_jumps=False):
    """
    ``expected_history`` for every model: the exact expected dwell times and numbers of Markov jumps under the posterior over
    whole histories, for characters under the F81 family, the eigen models (JTT, CUSTOM_RATES) and HKY alike.

    Characters are grouped by their number of states and by path; a group is one batch on the device.  F81-family characters
    take ``expected_history``'s path (``pml_expected_history``) and their results are its results bit for bit.  Eigen models
    take the eigenbasis integral of Minin & Suchard / Hobolth & Jensen over the vectors of the marginal pass
    (``pml_expected_history_eigen``, HIP; include/pastml_hip.h has the sums; 2 to 256 states; no P(t), memory O(N k)).  HKY
    runs as an eigen model, built from ``HKYModel.eigen_spec()``: its ``log_likelihood`` is then that of the eigen sweeps, which
    agrees with the closed-form HKY sweep to rounding, not bit for bit.  The sums of the eigen path have mixed signs: an entry
    that rounding leaves below zero is returned as 0.

    The file-level front end and sharding over ranks are not covered.  Parameters and return values are ``expected_history``'s.
    """
    from pastml_amd import sharding
    from pastml_amd.batch import CharacterBatch, LikelihoodError, annotation_words, likelihood_error
    from pastml_amd.models import KIND_F81, KIND_HKY
    if isinstance(forest, TreeNode):
        forest = [forest]
    single = isinstance(characters, str)
    if single:
        characters, models = [characters], [models]
    characters, models = list(characters), list(models)
    if len(characters) != len(models):
        raise ValueError('one model per character expected')
    world = sharding.rank_world()[1]
    if world > 1:
        raise NotImplementedError('expected_history_general is not supported under a multi-process launch ({} ranks): run it in '
                                  'a single process'.format(world))
    flat = get_flat_forest(forest)
    groups = {}
    for i, model in enumerate(models):
        kind = model.kernel_spec()['kind']
        groups.setdefault((len(model.states), kind == KIND_F81), []).append(i)
        if kind == KIND_HKY:
            models[i] = _AsEigenModel(model)
    results = [None] * len(characters)
    has_parent = flat.parent >= 0
    for (k, f81), members in groups.items():
        group_models = [models[i] for i in members]
        with CharacterBatch(flat, k, len(members)) as batch:
            for c, i in enumerate(members):
                batch.set_annotation(c, *annotation_words(flat, characters[i], models[i].states))
            batch.initialize_allowed_states()
            run = batch.expected_history if f81 else batch.expected_history_eigen
            try:
                lnl, times, jumps, per_branch = run(group_models, jumps=True, branch_jumps=branch_jumps)
            except LikelihoodError as e:
                raise likelihood_error(flat, e)
        for c, i in enumerate(members):
            _, tau, tau_factor = models[i].rate_params()
            result = dict(log_likelihood=float(lnl[c]), states=np.array(models[i].states), times=times[c].copy(),
                          jumps=jumps[c].copy(), tree_length=float(((flat.dist[has_parent] + tau) * tau_factor).sum()))
            if branch_jumps:
                result['branch_jumps'] = per_branch[c].copy()
            results[i] = result
    return results[0] if single else results


# =====================================================================================================================
# expected_history_through_time
# =====================================================================================================================

def time_bin_fractions(flat, node_times, boundaries):
    """
    float64 [M, N]: the fraction w of the branch above every node that lies in each time bin, formed as the segment plan of
    ``pml_history_through_time`` forms it: (min(T_m+1, time_n) - max(T_m, time_p)) / (time_n - time_p) where that is positive; a
    branch without extent counts whole in the bin that contains its time (the last bin contains the last boundary); a root: 0.
    """
    T = np.asarray(boundaries, dtype=np.float64)
    t = np.asarray(node_times, dtype=np.float64)
    M = len(T) - 1
    has_parent = flat.parent >= 0
    tn = t
    tp = np.where(has_parent, t[np.maximum(flat.parent, 0)], t)
    h = tn - tp
    flat_branch = has_parent & (h == 0)
    safe = np.where(h > 0, h, 1.0)
    out = np.zeros((M, flat.n_nodes), dtype=np.float64)
    for m in range(M):
        lo, hi = np.maximum(T[m], tp), np.minimum(T[m + 1], tn)
        out[m] = np.where(has_parent & (h > 0) & (hi > lo), (hi - lo) / safe, 0.0)
        inside = (T[m] <= tn) & ((tn < T[m + 1]) | ((m == M - 1) & (tn == T[M])))
        out[m][flat_branch & inside] = 1.0
    return out


def expected_history_through_time(forest, characters, models, boundaries, root_dates=None, node_dates=None, jumps=True):
    """
    ``expected_history`` per time interval: the exact expected dwell time in each state and number of jumps i -> j inside every
    bin of a dated forest, and the expected number of lineages in each state at every boundary, for one character or a list of
    them under F81-family models (F81, JC, EFT) -- ``pml_history_through_time``, HIP; include/pastml_hip.h has the sums.  A
    branch that crosses a boundary is split inside the branch, in closed form; jumps divided by dwell time is a rate per interval.

    Node times come from ``pastml_amd.tree.annotate_dates(flat, root_dates, given=node_dates)``: the distance from the root
    where nothing is given.  Characters are grouped by their number of states; a group is one batch on the device: one marginal
    pass (masks altered where tau == 0, restored afterwards) and one pass over its columns.  HKY and the eigen models, the
    file-level front end and sharding over ranks are not covered.

    :param characters: a character (feature name) or a list of them; models: a model or a list, one per character
    :param boundaries: an ascending sequence T_0 < ... < T_M -- bin m is [T_m, T_m+1), the last one also contains T_M --, or an
        int M for M equal bins from the earliest root to the latest tip
    :param root_dates, node_dates: as ``annotate_dates`` takes them (node_dates: float64 [N] in FlatForest node order, NaN where
        no date is given)
    :param jumps: False leaves the jumps out (``jumps`` is None then)
    :return: per character a dict with ``log_likelihood``; ``states``; ``boundaries`` [M + 1]; ``times`` [M, k] in units of
        smoothed branch length ((dist + tau) * tau_factor), a row summing to its ``bin_length``; ``jumps`` [M, k, k], zero
        diagonals; ``lineages`` [M + 1, k], a row summing to the number of branches alive at that boundary; ``bin_length`` [M]:
        the smoothed tree length inside each bin; and ``tree_length``.
    """
    return _history_through_time('expected_history_through_time', False, forest, characters, models, boundaries, root_dates,
                                 node_dates, jumps)


def expected_history_through_time_general(forest, characters, models, boundaries, root_dates=None, node_dates=None, jumps=True):
    """
    ``expected_history_through_time`` for every model: the counterpart of ``expected_history_general``, for characters under the
    F81 family, the eigen models (JTT, CUSTOM_RATES) and HKY alike.

    Characters are grouped by their number of states and by path; a group is one batch on the device.  F81-family characters
    take ``expected_history_through_time``'s path (``pml_history_through_time``) and their results are its results bit for bit.
    Eigen models take ``expected_history_general``'s eigenbasis integral cut at the boundaries inside every branch
    (``pml_history_through_time_eigen``, HIP; include/pastml_hip.h has the sums; 2 to 256 states).  HKY runs as an eigen model,
    built from ``HKYModel.eigen_spec()``.  The sums of the eigen path have mixed signs: an entry that rounding leaves below zero is
    returned as 0.

    The file-level front end and sharding over ranks are not covered.  Parameters and return values are
    ``expected_history_through_time``'s.
    """
    return _history_through_time('expected_history_through_time_general', True, forest, characters, models, boundaries, root_dates,
                                 node_dates, jumps)


def _history_through_time(name, general, forest, characters, models, boundaries, root_dates, node_dates, jumps):
    """The two front ends above: ``general`` serves every model kind, else every kind but the F81 family is refused by name."""
    from pastml_amd import sharding
    from pastml_amd.batch import CharacterBatch, LikelihoodError, annotation_words, likelihood_error
    from pastml_amd.models import KIND_F81, KIND_HKY
    from pastml_amd.tree import annotate_dates
    if isinstance(forest, TreeNode):
        forest = [forest]
    single = isinstance(characters, str)
    if single:
        characters, models = [characters], [models]
    characters, models = list(characters), list(models)
    if len(characters) != len(models):
        raise ValueError('one model per character expected')
    kinds = [model.kernel_spec()['kind'] for model in models]
    for character, model, kind in zip(characters, models, kinds):
        if not general and kind != KIND_F81:
            raise NotImplementedError('Character {}: expected_history_through_time is for the F81 family (F81, JC, EFT), not for {} '
                                      '(PML_ERR_UNSUPPORTED).'.format(character, getattr(model, 'name', type(model).__name__)))
    world = sharding.rank_world()[1]
    if world > 1:
        raise NotImplementedError('{} is not supported under a multi-process launch ({} ranks): run it in a single '
                                  'process'.format(name, world))
    flat = get_flat_forest(forest)
    node_times = annotate_dates(flat, root_dates, given=node_dates)
    if isinstance(boundaries, (int, np.integer)):
        if boundaries < 1:
            raise ValueError('at least one time bin is needed')
        boundaries = np.linspace(node_times[flat.parent < 0].min(), node_times[flat.tips].max(), int(boundaries) + 1)
    boundaries = np.array(boundaries, dtype=np.float64)
    if boundaries.ndim != 1 or len(boundaries) < 2 or not np.isfinite(boundaries).all() or not (np.diff(boundaries) > 0).all():
        raise ValueError('boundaries must be two or more finite, strictly ascending numbers')
    groups = {}
    for i, (model, kind) in enumerate(zip(models, kinds)):
        groups.setdefault((len(model.states), kind == KIND_F81), []).append(i)
        if kind == KIND_HKY:
            models[i] = _AsEigenModel(model)
    results = [None] * len(characters)
    has_parent = flat.parent >= 0
    fractions = time_bin_fractions(flat, node_times, boundaries)
    for (k, f81), members in groups.items():
        group_models = [models[i] for i in members]
        with CharacterBatch(flat, k, len(members)) as batch:
            for c, i in enumerate(members):
                batch.set_annotation(c, *annotation_words(flat, characters[i], models[i].states))
            batch.initialize_allowed_states()
            run = batch.history_through_time if f81 else batch.history_through_time_eigen
            try:
                lnl, times, jumps_out, lineages = run(group_models, node_times, boundaries, jumps=jumps)
            except LikelihoodError as e:
                raise likelihood_error(flat, e)
        for c, i in enumerate(members):
            _, tau, tau_factor = models[i].rate_params()
            length = np.where(has_parent, (flat.dist + tau) * tau_factor, 0.0)
            results[i] = dict(log_likelihood=float(lnl[c]), states=np.array(models[i].states), boundaries=boundaries.copy(),
                              times=times[c].copy(), jumps=None if jumps_out is None else jumps_out[c].copy(),
                              lineages=lineages[c].copy(), bin_length=fractions.dot(length),
                              tree_length=float(((flat.dist[has_parent] + tau) * tau_factor).sum()))
    return results[0] if single else results
