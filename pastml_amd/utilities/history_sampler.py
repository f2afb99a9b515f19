"""
Stochastic character maps on the GPU: whole histories of a character -- every change along every branch and the time spent in
each state -- drawn from their posterior given the tips, under the F81 family (F81, JC, EFT): ``pml_sample_histories``.

``expected_history`` gives the posterior means of the dwell times and of the Markov jumps in closed form; ``sample_scenarios``
draws the states at the nodes.  Here each sampled scenario is completed by a history on every branch between its two end
states, so that the number of A -> B events (those undone on the same branch included) or the share of the tree spent in a
state get a distribution, not only a mean: ``history_summary`` puts the mean and a credible interval of every entry next to
``expected_history``'s.  ``sample_histories_through_time`` cuts the same histories at the boundaries of time bins of a dated
forest (``pml_sample_histories_through_time``) and ``history_time_summary`` sets them next to
``expected_history_through_time``, with a rate per interval.
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


# =====================================================================================================================
# per time interval
# =====================================================================================================================

def _time_segments(flat, node_times, boundaries):
    """The number of segments of the plan of ``pml_sample_histories_through_time`` (pml_time_segments.h): per branch with
    extent one for every bin it overlaps, one for a branch without extent whose time a bin contains."""
    T = np.asarray(boundaries, dtype=np.float64)
    t = np.asarray(node_times, dtype=np.float64)
    has_parent = flat.parent >= 0
    tn, tp = t[has_parent], t[flat.parent[has_parent]]
    total = 0
    for m in range(len(T) - 1):
        total += int(((np.minimum(T[m + 1], tn) > np.maximum(T[m], tp)) & (tn > tp)).sum())
    total += int(((tn == tp) & (T[0] <= tn) & (tn <= T[-1])).sum())
    return total


def _time_pieces(n_nodes, n_segments, n_bins):
    """At most this many pieces of segments (pml_launch_history_time_sample.hip: pieces of as many segments as
    ``sample_histories``' pieces have ids, cut per bin, so that every bin may add a ragged one)."""
    piece = 64 * ((max(64, (n_nodes + 255) // 256) + 63) // 64)
    return (n_segments + piece - 1) // piece + n_bins


def _bytes_per_repetition_through_time(n_nodes, k, n_bins, n_segments, jumps, lineages):
    """Device memory one repetition of a call takes: its states, its times [M, k] and their partials (one row of k per piece),
    its uint32 jump tables [M, k, k] and its uint32 lineage counts [M + 1, k], where asked for."""
    states = n_nodes * (1 if k <= 256 else 2)
    times = (n_bins + _time_pieces(n_nodes, n_segments, n_bins)) * k * 8
    return states + times + (n_bins * k * k * 4 if jumps else 0) + ((n_bins + 1) * k * 4 if lineages else 0)


def sample_histories_through_time(forest, character, model, boundaries, n_repetitions=1_000, root_dates=None, node_dates=None,
                                  jumps=True, lineages=True):
    """
    ``sample_histories`` per time interval: the sampled counterpart of ``ml.expected_history_through_time``.  Every repetition is
    the history ``sample_histories`` draws for the same seed, with its events placed on the branches and cut at the boundaries
    of the time bins of a dated forest (``pml_sample_histories_through_time``; include/pastml_hip.h states the law): the time
    spent in each state and the jumps i -> j inside every bin, and the lineages in each state at every boundary -- draws, so
    that the rate of A -> B in one period can be set against another with a credible interval (``history_time_summary``).

    Node times come from ``pastml_amd.tree.annotate_dates(flat, root_dates, given=node_dates)``.  Every node gets the feature
    ``character`` as ``sample_scenarios`` attaches it.  The draws are seeded from numpy's global generator; the repetitions are
    drawn in chunks sized from the device's free memory.  HKY and the eigen models and sharding over ranks are not covered.

    :param boundaries: an ascending sequence T_0 < ... < T_M -- bin m is [T_m, T_m+1), the last one also contains T_M --, or an
        int M for M equal bins from the earliest root to the latest tip
    :param jumps, lineages: False leaves them out (None then)
    :return: dict with ``states`` (``model.states``); ``boundaries`` [M + 1]; ``times`` [n_repetitions, M, k] in units of smoothed
        branch length; ``jumps`` [n_repetitions, M, k, k] uint32, zero diagonals, or None; ``lineages`` [n_repetitions, M + 1, k]
        uint32, a row summing to the number of branches alive at that boundary, or None; ``bin_length`` [M]: the smoothed tree
        length inside each bin, what a row of ``times`` sums to; ``tree_length``.
    """
    from pastml_amd.ml import time_bin_fractions
    from pastml_amd.tree import annotate_dates
    trees = [forest] if isinstance(forest, TreeNode) else list(forest)
    k = len(model.states)
    name = getattr(model, 'name', type(model).__name__)
    n_repetitions = int(n_repetitions)
    if n_repetitions < 1:
        raise ValueError('Character {}: n_repetitions must be at least 1 to sample its histories through time under {}, got {}.'
                         .format(character, name, n_repetitions))
    if name not in (F81, JC, EFT):
        raise NotImplementedError('Character {}: sample_histories_through_time is for the F81 family (F81, JC, EFT), not for {} '
                                  '(PML_ERR_UNSUPPORTED).'.format(character, name))
    if k > hip.MAX_STATES:
        raise ValueError('Character {} has {} states: the MI355X history sampler supports at most {} states per character '
                         'under {} (PML_ERR_UNSUPPORTED); merge rare states.'.format(character, k, hip.MAX_STATES, name))
    world = sharding.rank_world()[1]
    if world > 1:
        raise NotImplementedError('sample_histories_through_time is not supported under a multi-process launch ({} ranks): the '
                                  'histories of a character are arrays on one device; run it in a single process'.format(world))
    problem = ForestProblem(trees, character, model.states)
    try:
        flat = problem.flat
        node_times = annotate_dates(flat, root_dates, given=node_dates)
        if isinstance(boundaries, (int, np.integer)):
            if boundaries < 1:
                raise ValueError('at least one time bin is needed')
            boundaries = np.linspace(node_times[flat.parent < 0].min(), node_times[flat.tips].max(), int(boundaries) + 1)
        boundaries = np.array(boundaries, dtype=np.float64)
        if boundaries.ndim != 1 or len(boundaries) < 2 or not np.isfinite(boundaries).all() or not (np.diff(boundaries) > 0).all():
            raise ValueError('boundaries must be two or more finite, strictly ascending numbers')
        M = len(boundaries) - 1
        problem.initialize_allowed_states()
        if 0 == model.tau:
            problem.alter_zero_node_allowed_states()
        problem.bottom_up_loglikelihood(model, is_marginal=True, alter=False)
        problem.top_down_marginals()
        engine = problem.engine
        seed = int(np.random.randint(0, 2 ** 62, dtype=np.int64))
        n = flat.n_nodes
        states = np.empty((n, n_repetitions), dtype=np.uint8 if k <= 256 else np.uint16)
        times = np.empty((n_repetitions, M, k), dtype=np.float64)
        jumps_out = np.empty((n_repetitions, M, k, k), dtype=np.uint32) if jumps else None
        lineages_out = np.empty((n_repetitions, M + 1, k), dtype=np.uint32) if lineages else None
        _, free = engine.memory()
        if os.environ.get('PASTML_AMD_DEVICE_BYTES'):   # plan as if the device had this much free memory (tests)
            free = min(free, int(float(os.environ['PASTML_AMD_DEVICE_BYTES'])))
        per_rep = _bytes_per_repetition_through_time(n, k, M, _time_segments(flat, node_times, boundaries), jumps, lineages)
        fit = int(_DEVICE_SHARE * max(0, free)) // per_rep
        chunk = int(min(n_repetitions, max(4, fit // 4 * 4)))
        sample_histories_through_time.last_stats = dict(repetitions_per_call=chunk, bytes_per_repetition=per_rep)
        n_fallback = 0
        for offset in range(0, n_repetitions, chunk):
            count = min(chunk, n_repetitions - offset)
            s, t, j, l, fallen = engine.sample_histories_through_time(node_times, boundaries, count, seed, rep_offset=offset,
                                                                      jumps=jumps, lineages=lineages, states=True)
            states[:, offset:offset + count] = s
            times[offset:offset + count] = t
            if jumps:
                jumps_out[offset:offset + count] = j
            if lineages:
                lineages_out[offset:offset + count] = l
            n_fallback += fallen
    finally:
        problem.close()
    if n_fallback:
        raise RuntimeError('Character {}: {} draws found no state with weight given their parent\'s state: the marginal pass '
                           'is not consistent with its masks.'.format(character, n_fallback))
    flat.set_column(character, ArrayColumn(states))
    _, tau, tau_factor = model.rate_params()
    has_parent = flat.parent >= 0
    length = np.where(has_parent, (flat.dist + tau) * tau_factor, 0.0)
    return dict(states=np.array(model.states), boundaries=boundaries.copy(), times=times, jumps=jumps_out, lineages=lineages_out,
                bin_length=time_bin_fractions(flat, node_times, boundaries).dot(length),
                tree_length=float(((flat.dist[has_parent] + tau) * tau_factor).sum()))


def history_time_summary(result, level=0.95):
    """
    Mean and central credible interval of every entry of ``sample_histories_through_time``'s times [M, k], jumps [M, k, k] and
    lineages [M + 1, k] over the repetitions (None where the result has none), to be set next to
    ``ml.expected_history_through_time``: dict with ``level``, ``n_repetitions``, ``states``, ``boundaries`` and, for each, a dict of
    ``mean``, ``lower`` and ``upper`` (the (1 - level) / 2 and (1 + level) / 2 quantiles).  ``rates`` [M, k, k] likewise, with
    ``kept``: entry [m, i, j] is jumps[r, m, i, j] / times[r, m, i] per repetition, over the repetitions that spend time in state
    i in bin m; those with a zero dwell are left out of that entry, ``kept`` says how many stayed, and an entry that keeps none
    is NaN.  None without jumps.
    """
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError('level must lie between 0 and 1, got {}'.format(level))
    tail = (1.0 - level) / 2.0

    def summary(values):
        if values is None:
            return None
        values = np.asarray(values, dtype=np.float64)
        lower, upper = np.quantile(values, [tail, 1.0 - tail], axis=0)
        return dict(mean=values.mean(axis=0), lower=lower, upper=upper)

    times = np.asarray(result['times'], dtype=np.float64)
    rates = None
    if result['jumps'] is not None:
        spent = times > 0.0                                                   # [R, M, k]
        with np.errstate(divide='ignore', invalid='ignore'):
            per_rep = np.where(spent[..., None], np.asarray(result['jumps'], dtype=np.float64) / times[..., None], np.nan)
        kept = np.broadcast_to(spent.sum(axis=0)[..., None], per_rep.shape[1:]).copy()
        some = kept > 0
        safe = np.where(some[None], per_rep, 0.0)                             # (an entry that keeps none: NaN below, no warning)
        lower, upper = np.nanquantile(safe, [tail, 1.0 - tail], axis=0)
        mean = np.nansum(safe, axis=0) / np.maximum(kept, 1)
        rates = dict(mean=np.where(some, mean, np.nan), lower=np.where(some, lower, np.nan), upper=np.where(some, upper, np.nan),
                     kept=kept)
    return dict(level=level, n_repetitions=int(times.shape[0]), states=result['states'], boundaries=result['boundaries'],
                times=summary(times), jumps=summary(result['jumps']), lineages=summary(result['lineages']), rates=rates)
