"""
Forward simulation of a character along a forest under a model (API of pastml/utilities/state_simulator.py:6-31), on the
GPU: ``pml_simulate_states``.
"""
import os

import numpy as np

from pastml_amd import hip
from pastml_amd.models._closed_form import EFT, F81, JC
from pastml_amd.tree import ArrayColumn, TreeNode, get_flat_forest

# share of the device's free memory the [N, repetitions] state buffer of one call may take
_DEVICE_SHARE = 0.5


def _reserved_bytes(n_nodes, k, matrix, window=0):
    """
    Device memory the first call allocates besides the states: for the models with a P(t) matrix per branch, the P(t)
    batch of the column (k x ks doubles per node; the library pads ks to a multiple of at most 8) -- or, where a window of
    P(t) is planned (``window`` branches, batch.plan_consumer_window), that window and the lists of the windowed schedule --
    and, beyond 128 states, the scratch of the cumulative rows (at most 256 MB, pml_launch_simulate.hip).
    """
    if not matrix:
        return 0
    ks = (k + 7) // 8 * 8
    held = window * k * ks * 8 + 24 * n_nodes if window else n_nodes * k * ks * 8
    return held + ((256 << 20) if k > 128 else 0)


def _chunk(n_nodes, n_repetitions, bytes_per_state, free):
    """Repetitions per device call: the call's state buffer within a share of the free memory (a multiple of 4)."""
    fit = int(_DEVICE_SHARE * max(0, free)) // max(1, n_nodes * bytes_per_state)
    return int(min(n_repetitions, max(4, fit // 4 * 4)))


def _window_and_chunk(flat, k, matrix, window, n_repetitions, bytes_per_state, free):
    """
    (branches of the window, repetitions per device call).  Every chunk of repetitions builds P(t) of the whole tree once, run
    by run, so under a window one larger chunk is preferred over more chunks: where the repetitions do not fit one call beside
    the planned window, the window gives way down to batch.PIJ_WINDOW_PREFERRED branches (never below the largest fan-out).
    """
    from pastml_amd.batch import PIJ_WINDOW_PREFERRED
    n, itemsize = flat.n_nodes, bytes_per_state
    chunk = _chunk(n, n_repetitions, itemsize, free - _reserved_bytes(n, k, matrix, window))
    if window and chunk < n_repetitions:
        smaller = max(int(np.max(flat.n_children)), min(window, PIJ_WINDOW_PREFERRED))
        if smaller < window:
            window = smaller
            chunk = _chunk(n, n_repetitions, itemsize, free - _reserved_bytes(n, k, matrix, window))
    return window, chunk


def simulate_states(tree, model, character, n_repetitions=1_000):
    """
    Simulates n_repetitions scenarios of the character along the tree (or list of trees): each root draws from
    ``model.frequencies``, each other node from row a of ``model.get_Pij_t(n.dist)`` (negatives clamped to 0), a being its
    parent's state.  State ids index ``model.states``.  Every node gets the feature ``character``: an integer array of
    length n_repetitions, a row of one [N, n_repetitions] array held as a column of the forest.

    The draws are the device's (Philox-4x32-10), seeded from numpy's global generator: ``np.random.seed`` fixes the result.
    Only statistical parity with the reference's numpy draws is meaningful.

    :return: the tree (or list of trees) it was given
    """
    forest = [tree] if isinstance(tree, TreeNode) else list(tree)
    k = len(model.states)
    name = getattr(model, 'name', type(model).__name__)
    n_repetitions = int(n_repetitions)
    if n_repetitions < 1:
        raise ValueError('Character {}: n_repetitions must be at least 1 to simulate it under {}, got {}.'
                         .format(character, name, n_repetitions))
    matrix = name not in (F81, JC, EFT)
    most = hip.MAX_STATES_MATRIX if matrix else hip.MAX_STATES
    if k > most:
        raise ValueError('Character {} has {} states: the MI355X simulator supports at most {} states per character under {} '
                         '(PML_ERR_UNSUPPORTED); merge rare states.'.format(character, k, most, name))
    from pastml_amd.batch import consumer_window
    flat = get_flat_forest(forest)
    # a character whose whole-tree batch of P(t) does not fit the device is simulated with a window of it (MemoryError if
    # not even the smallest window fits)
    window, record = consumer_window(flat, k, model.kernel_spec()['kind'], 1, character, 'simulate_states')
    seed = int(np.random.randint(0, 2 ** 62, dtype=np.int64))
    dtype = np.uint8 if k <= 256 else np.uint16
    states = np.empty((flat.n_nodes, n_repetitions), dtype=dtype)
    with hip.Engine(flat, 1, k) as engine:
        engine.set_models([model])
        _, free = engine.memory()
        if os.environ.get('PASTML_AMD_DEVICE_BYTES'):   # plan as if the device had this much free memory (tests)
            free = min(free, int(float(os.environ['PASTML_AMD_DEVICE_BYTES'])))
        # (the batch or the window: not allocated before the first call / allocated right below)
        window, chunk = _window_and_chunk(flat, k, matrix, window, n_repetitions, np.dtype(dtype).itemsize, free)
        if window:
            engine.pij_window_set(window)
        record.update(branches=window, repetitions_per_call=chunk)
        simulate_states.last_stats = dict(pij_window=[record])
        for offset in range(0, n_repetitions, chunk):
            count = min(chunk, n_repetitions - offset)
            states[:, offset:offset + count] = engine.simulate_states(count, seed, rep_offset=offset)
    flat.set_column(character, ArrayColumn(states))
    return tree
