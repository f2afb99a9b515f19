"""
Stochastic character maps on the GPU: whole histories of a character -- every change along every branch and the time spent in
each state -- drawn from their posterior given the tips, under the F81 family (F81, JC, EFT): ``pml_sample_histories``.

``expected_history`` gives the posterior means of the dwell times and of the Markov jumps in closed form; ``sample_scenarios``
draws the states at the nodes.  Here each sampled scenario is completed by a history on every branch between its two end
states, so that the number of A -> B events (those undone on the same branch included) or the share of the tree spent in a
state get a distribution, not only a mean: ``history_summary`` puts the mean and a credible interval of every entry next to
``expected_history``'s.
"""
import os

import numpy as np

from pastml_amd import hip, sharding
from pastml_amd.ml import ForestProblem
from pastml_amd.models._closed_form import EFT, F81, JC
from pastml_amd.tree import ArrayColumn, TreeNode

# share of the device's free memory the buffers of one call may take
_DEVICE_SHARE = 0.5


def _pieces(n_nodes):
    """Pieces of node ids the device walks (pml_launch_history_sample.hip: 64 ceil(max(64, ceil(N / 256)) / 64) ids each)."""
    piece = 64 * ((max(64, (n_nodes + 255) // 256) + 63) // 64)
    return (n_nodes + piece - 1) // piece


def _bytes_per_repetition(n_nodes, k, branch_jumps):
    """Device memory one repetition of a call takes: its states, its times and their partials (one row per piece), its uint32
    jump table and, if asked for, its uint16 branch counts."""
    states = n_nodes * (1 if k <= 256 else 2)
    times = (1 + _pieces(n_nodes)) * k * 8
    return states + times + k * k * 4 + (2 * n_nodes if branch_jumps else 0)


def _chunk(n_nodes, k, n_repetitions, branch_jumps, free):
    """Repetitions per device call: the call's buffers within a share of the free memory (a multiple of 4)."""
    fit = int(_DEVICE_SHARE * max(0, free)) // _bytes_per_repetition(n_nodes, k, branch_jumps)
    return int(min(n_repetitions, max(4, fit // 4 * 4)))


def sample_histories(forest, character, model, n_repetitions=1_000, branch_jumps=False):
    """
    Draws n_repetitions histories of the character from their posterior given the tips.  The marginal pass runs on the device
    as for ``sample_scenarios`` and the scenarios are the ones it would draw for the same seed; then, per branch and repetition,
    the number of redraw events of the F81 process between the two end states (a zero-truncated Poisson, or none with a known
    probability when the ends agree), the states they redraw (independent draws from the frequencies, the last one the child's
    state) and their times (uniform) are drawn -- no rejection, no matrix (include/pastml_hip.h states the law draw by draw).
    Events that redraw the state they find are not jumps and count nowhere.

    Every node gets the feature ``character`` as ``sample_scenarios`` attaches it: its state in every repetition.  The draws
    are the device's (Philox-4x32-10), seeded from numpy's global generator: ``np.random.seed`` fixes the result.  The
    repetitions are drawn in chunks sized from the device's free memory.

    :param branch_jumps: also return the number of jumps on the branch above every node
    :return: dict with ``states`` (``model.states``); ``times`` [n_repetitions, k]: the time spent in each state, in units of
        smoothed branch length ((dist + tau) * tau_factor), every row summing to ``tree_length``; ``jumps`` [n_repetitions, k, k]
        uint32: entry [r, i, j] = number of jumps i -> j in repetition r, zero diagonal; ``branch_jumps`` [N, n_repetitions]
        uint16 in FlatForest node order (0 for a root) or None; ``tree_length``.
    """
    trees = [forest] if isinstance(forest, TreeNode) else list(forest)
    k = len(model.states)
    name = getattr(model, 'name', type(model).__name__)
    n_repetitions = int(n_repetitions)
    if n_repetitions < 1:
        raise ValueError('Character {}: n_repetitions must be at least 1 to sample its histories under {}, got {}.'
                         .format(character, name, n_repetitions))
    if name not in (F81, JC, EFT):
        raise NotImplementedError('Character {}: sample_histories is for the F81 family (F81, JC, EFT), not for {} '
                                  '(PML_ERR_UNSUPPORTED).'.format(character, name))
    if k > hip.MAX_STATES:
        raise ValueError('Character {} has {} states: the MI355X history sampler supports at most {} states per character '
                         'under {} (PML_ERR_UNSUPPORTED); merge rare states.'.format(character, k, hip.MAX_STATES, name))
    world = sharding.rank_world()[1]
    if world > 1:
        raise NotImplementedError('sample_histories is not supported under a multi-process launch ({} ranks): the histories '
                                  'of a character are arrays on one device; run it in a single process'.format(world))
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
        n = flat.n_nodes
        states = np.empty((n, n_repetitions), dtype=np.uint8 if k <= 256 else np.uint16)
        times = np.empty((n_repetitions, k), dtype=np.float64)
        jumps = np.empty((n_repetitions, k, k), dtype=np.uint32)
        per_branch = np.empty((n, n_repetitions), dtype=np.uint16) if branch_jumps else None
        _, free = engine.memory()
        if os.environ.get('PASTML_AMD_DEVICE_BYTES'):   # plan as if the device had this much free memory (tests)
            free = min(free, int(float(os.environ['PASTML_AMD_DEVICE_BYTES'])))
        chunk = _chunk(n, k, n_repetitions, branch_jumps, free)
        sample_histories.last_stats = dict(repetitions_per_call=chunk, bytes_per_repetition=_bytes_per_repetition(n, k, branch_jumps))
        n_fallback = 0
        for offset in range(0, n_repetitions, chunk):
            count = min(chunk, n_repetitions - offset)
            s, t, j, b, fallen = engine.sample_histories(count, seed, rep_offset=offset, jumps=True, branch_jumps=branch_jumps,
                                                         states=True)
            states[:, offset:offset + count] = s
            times[offset:offset + count] = t
            jumps[offset:offset + count] = j
            if branch_jumps:
                per_branch[:, offset:offset + count] = b
            n_fallback += fallen
    finally:
        problem.close()
    if n_fallback:
        raise RuntimeError('Character {}: {} draws found no state with weight given their parent\'s state: the marginal pass '
                           'is not consistent with its masks.'.format(character, n_fallback))
    flat.set_column(character, ArrayColumn(states))
    _, tau, tau_factor = model.rate_params()
    return dict(states=np.array(model.states), times=times, jumps=jumps, branch_jumps=per_branch,
                tree_length=float(((flat.dist[flat.parent >= 0] + tau) * tau_factor).sum()))


def history_summary(result, level=0.95):
    """
    Mean and central credible interval of every entry of ``sample_histories``' times and jumps over the repetitions, to be set
    next to ``expected_history``: dict with ``level``, ``n_repetitions`` and, for ``times`` [k] and ``jumps`` [k, k] each, a dict
    of ``mean``, ``lower`` and ``upper`` (the (1 - level) / 2 and (1 + level) / 2 quantiles), and ``time_share`` likewise: the
    times over ``tree_length``.
    """
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError('level must lie between 0 and 1, got {}'.format(level))
    tail = (1.0 - level) / 2.0

    def summary(values):
        values = np.asarray(values, dtype=np.float64)
        lower, upper = np.quantile(values, [tail, 1.0 - tail], axis=0)
        return dict(mean=values.mean(axis=0), lower=lower, upper=upper)

    times = np.asarray(result['times'], dtype=np.float64)
    return dict(level=level, n_repetitions=int(times.shape[0]), states=result['states'], times=summary(times),
                jumps=summary(result['jumps']), time_share=summary(times / float(result['tree_length'])))
