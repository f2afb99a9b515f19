"""
Ancestral scenarios drawn from the joint posterior of a character given the tips, on the GPU: ``pml_sample_scenarios``.

``marginal_counts`` samples the same law but keeps only a k x k table, ``expected_counts`` gives that table's mean, and
``simulate_states`` draws whole scenarios from the prior.  Here the scenarios themselves come back: complete, internally
consistent histories, from which a credible interval on the number of A -> B changes, the distribution of the first node in
a state along a lineage or any other functional can be computed.
"""
import os

import numpy as np

from pastml_amd import hip, sharding
from pastml_amd.ml import ForestProblem
from pastml_amd.models._closed_form import EFT, F81, JC
from pastml_amd.tree import ArrayColumn, TreeNode
from pastml_amd.utilities.state_simulator import _window_and_chunk


def sample_scenarios(forest, character, model, n_repetitions=1_000):
    """
    Draws n_repetitions ancestral scenarios of the character from their joint posterior (the sampling scheme of
    pastml/ml.py:786-824, per repetition): the marginal pass runs on the device as for ``marginal_counts``; then every root
    draws from its marginal posterior and every other node b from ``BU_n[b] * pi_b * mask_n[b] * P_n[b][a]``, a being its
    parent's state in the same repetition.  The masks are the ones the pass ran with: with ``model.tau == 0`` those altered by
    the zero-branch handling, so a node at the end of a zero branch may take a state of its neighbours.

    Every node gets the feature ``character`` (its annotation is replaced): an integer array of length n_repetitions, a row
    of one [N, n_repetitions] array held as a column of the forest (uint8 up to 256 states, else uint16); state ids index
    ``model.states``.  The draws are the device's (Philox-4x32-10), seeded from numpy's global generator: ``np.random.seed``
    fixes the result.  The repetitions are drawn in chunks sized from the device's free memory.

    :return: the forest (or tree) it was given
    """
    trees = [forest] if isinstance(forest, TreeNode) else list(forest)
    k = len(model.states)
    name = getattr(model, 'name', type(model).__name__)
    n_repetitions = int(n_repetitions)
    if n_repetitions < 1:
        raise ValueError('Character {}: n_repetitions must be at least 1 to sample its scenarios under {}, got {}.'
                         .format(character, name, n_repetitions))
    matrix = name not in (F81, JC, EFT)
    most = hip.MAX_STATES_MATRIX if matrix else hip.MAX_STATES
    if k > most:
        raise ValueError('Character {} has {} states: the MI355X scenario sampler supports at most {} states per character '
                         'under {} (PML_ERR_UNSUPPORTED); merge rare states.'.format(character, k, most, name))
    world = sharding.rank_world()[1]
    if world > 1:
        raise NotImplementedError('sample_scenarios is not supported under a multi-process launch ({} ranks): the scenarios '
                                  'of a character are one array on one device; run it in a single process'.format(world))
    problem = ForestProblem(trees, character, model.states)
    try:
        flat = problem.flat
        problem.initialize_allowed_states()
        if 0 == model.tau:
            problem.alter_zero_node_allowed_states()
        problem.bottom_up_loglikelihood(model, is_marginal=True, alter=False)
        problem.top_down_marginals()
        engine = problem.engine
        seed = int(np.random.randint(0, 2 ** 62, dtype=np.int64))
        dtype = np.uint8 if k <= 256 else np.uint16
        states = np.empty((flat.n_nodes, n_repetitions), dtype=dtype)
        _, free = engine.memory()
        if os.environ.get('PASTML_AMD_DEVICE_BYTES'):   # plan as if the device had this much free memory (tests)
            free = min(free, int(float(os.environ['PASTML_AMD_DEVICE_BYTES'])))
        # (the fused sweeps leave the batch of P(t) to the first call; a window is the context's already and is charged instead:
        # ForestProblem planned it before the first sweep)
        record = dict(problem.pij_window_stats)
        window, chunk = _window_and_chunk(flat, k, matrix, record['branches'], n_repetitions, np.dtype(dtype).itemsize,
                                          free + record['branches'] * k * ((k + 7) // 8 * 8) * 8)
        if window != record['branches']:
            engine.pij_window_set(window)   # (a smaller window for fewer chunks of repetitions: the pass's results stay)
        record.update(branches=window, repetitions_per_call=chunk)
        sample_scenarios.last_stats = dict(pij_window=[record])
        n_fallback = 0
        for offset in range(0, n_repetitions, chunk):
            count = min(chunk, n_repetitions - offset)
            states[:, offset:offset + count], fallen = engine.sample_scenarios(count, seed, rep_offset=offset)
            n_fallback += fallen
    finally:
        problem.close()
    if n_fallback:
        raise RuntimeError('Character {}: {} draws found no state with weight given their parent\'s state: the marginal pass '
                           'is not consistent with its masks.'.format(character, n_fallback))
    flat.set_column(character, ArrayColumn(states))
    return forest


def scenario_transition_counts(forest, character, k):
    """
    Numbers of a -> b (parent, child) pairs of every scenario that ``sample_scenarios`` attached as ``character``:
    [n_repetitions, k, k], entry [r, a, b] counting the branches whose parent is in state a and whose child is in state b in
    repetition r (the diagonal counts the branches without a change).  Quantiles over r give credible intervals.
    """
    from pastml_amd.tree import get_flat_forest
    trees = [forest] if isinstance(forest, TreeNode) else list(forest)
    flat = get_flat_forest(trees)
    states = np.stack([np.asarray(getattr(flat.nodes[i], character)) for i in range(flat.n_nodes)]).astype(np.int64)
    parent = np.asarray(flat.parent, dtype=np.int64)
    child = np.flatnonzero(parent >= 0)
    n_rep = states.shape[1]
    pair = states[parent[child]] * k + states[child]            # [branches, n_rep]
    pair += np.arange(n_rep, dtype=np.int64)[None, :] * (k * k)
    return np.bincount(pair.ravel(), minlength=n_rep * k * k).reshape(n_rep, k, k)
