"""Which refusal wins: the eleven entries that read a marginal pass (csrc/pml_api_readers.hip), as one table.

Rows: the entries.  Columns: the states of the context and the arguments an entry can be refused for -- no model set; a model
but no marginal pass; a marginal bottom-up sweep only; the wrong model kind (an eigen context for the entries of the F81 family,
an F81 context for pml_expected_history_eigen); a column out of range; n_repetitions = 0; rep_offset = -1; and two at once: no
pass and a bad column, the wrong kind and no pass.  Cells: the status and the whole message (none of them carries the file:line
tail of a failed HIP call), or OK where the entry runs -- pml_simulate_states needs a model and no pass.  A column that does
not apply to an entry has no cell.

The cells were written from the source of the commit before the entries moved into a translation unit of their own, in the
order their checks stood there, and the table was run once against that commit's library: what it pins is that the move did
not change which of two refusals a caller sees.  Nothing here is launched that could fault: every refused call returns before
its first launch.

A balanced tree of 8 tips, two columns, k = 4, one F81 and one eigen context: the smallest forest every entry runs on."""
import ctypes

import numpy as np
import pytest

from pastml_amd import hip, synthetic
from test_gpu_parity import random_spec

pytestmark = pytest.mark.gpu

K, C, LEVELS = 4, 2, 3
INVALID, UNSUPPORTED = hip.PML_ERR_INVALID, hip.PML_ERR_UNSUPPORTED
OK = (hip.PML_OK, '')
COLUMNS = ['no model', 'no pass', 'bottom-up only', 'wrong kind', 'bad column', 'n_repetitions = 0', 'rep_offset = -1',
           'no pass + bad column', 'wrong kind + no pass']


# ---------------------------------------------------------------------------------------------------------------------
# the cells
# ---------------------------------------------------------------------------------------------------------------------
NO_MODEL = (INVALID, 'model parameters of column 0 were never set')
RANGE = (INVALID, 'column range [0, 3) out of 0..2')
NOT_EIGEN = (UNSUPPORTED, "pml_expected_history_eigen is for the eigen-decomposed models: this context's model kind is F81 (F81, JC, "
                          "EFT), which pml_expected_history serves")


def _no_pass(name):
    return INVALID, name + ' needs a marginal pml_bottom_up and pml_top_down_marginals first'


def _not_f81(name):
    return UNSUPPORTED, name + " is for the F81 family (F81, JC, EFT): this context's model kind is eigen"


def _range_row(name, kind=None):
    """An entry over the columns [col_begin, col_end): the range is checked right behind the model, the kind ahead of the pass."""
    row = {'no model': NO_MODEL, 'no pass': _no_pass(name), 'bottom-up only': _no_pass(name), 'bad column': RANGE,
           'no pass + bad column': RANGE}
    if kind is not None:
        row['wrong kind'] = row['wrong kind + no pass'] = NOT_EIGEN if kind == 'eigen' else _not_f81(name)
    return row


def _draws_row(name, prefix, kind=None, pass_name=None, rep_offset=True, needs_pass=True):
    """An entry that draws n_repetitions of one column: column and outputs, n_repetitions, rep_offset -- in that order, all ahead
    of the kind and of the pass."""
    bad_column = (INVALID, prefix + 'bad column / output')
    missing = _no_pass(pass_name or name) if needs_pass else OK
    row = {'no model': NO_MODEL, 'no pass': missing, 'bottom-up only': missing, 'bad column': bad_column,
           'n_repetitions = 0': (INVALID, prefix + 'n_repetitions must be positive'), 'no pass + bad column': bad_column}
    if rep_offset:
        row['rep_offset = -1'] = (INVALID, prefix + 'rep_offset must not be negative')
    if kind is not None:
        row['wrong kind'] = row['wrong kind + no pass'] = _not_f81(name)
    return row


TABLE = {
    'pml_marginal_counts': _draws_row('pml_marginal_counts', '', rep_offset=False),
    'pml_marginal_counts_altered': _draws_row('pml_marginal_counts_altered', '', pass_name='pml_marginal_counts', rep_offset=False),
    'pml_expected_counts': _range_row('pml_expected_counts'),
    'pml_loglik_gradient': _range_row('pml_loglik_gradient', 'f81'),
    'pml_expected_history': _range_row('pml_expected_history', 'f81'),
    'pml_expected_history_eigen': _range_row('pml_expected_history_eigen', 'eigen'),
    'pml_history_through_time': _range_row('pml_history_through_time', 'f81'),
    'pml_simulate_states': _draws_row('pml_simulate_states', '', needs_pass=False),
    'pml_sample_scenarios': _draws_row('pml_sample_scenarios', ''),
    'pml_sample_histories': _draws_row('pml_sample_histories', 'pml_sample_histories: ', 'f81'),
    'pml_sample_histories_through_time': _draws_row('pml_sample_histories_through_time', 'pml_sample_histories_through_time: ', 'f81'),
}
HOME = {name: 'eigen' if name == 'pml_expected_history_eigen' else 'f81' for name in TABLE}


# ---------------------------------------------------------------------------------------------------------------------
# the calls: every array an entry can write is there and large enough for the call to run
# ---------------------------------------------------------------------------------------------------------------------
def _buffers(n_nodes):
    big = 4096
    assert big >= C * n_nodes * K * K
    return dict(f64=[np.zeros(big) for _ in range(3)], i32=[np.zeros(big, dtype=np.int32) for _ in range(2)],
                u32=[np.zeros(big, dtype=np.uint32) for _ in range(2)], u16=np.zeros(big, dtype=np.uint16),
                states=np.zeros(big, dtype=np.uint8), fallen=np.zeros(1, dtype=np.int64), altered=np.zeros(n_nodes, dtype=np.uint8),
                node_time=np.zeros(n_nodes), boundaries=np.array([0.0, 1.0]))


def _call(lib, ctx, name, b, cb=0, ce=C, col=0, n=4, off=0, seed=7):
    def p(arr, ctype):
        return arr.ctypes.data_as(ctypes.POINTER(ctype))

    dbl, i32, u32 = ctypes.c_double, ctypes.c_int32, ctypes.c_uint32
    f0, f1, f2 = (p(a, dbl) for a in b['f64'])
    states, fallen = b['states'].ctypes.data, p(b['fallen'], ctypes.c_int64)
    node_time, boundaries = p(b['node_time'], dbl), p(b['boundaries'], dbl)
    calls = {
        'pml_marginal_counts': lambda: lib.pml_marginal_counts(ctx, col, n, seed, f0),
        'pml_marginal_counts_altered': lambda: lib.pml_marginal_counts_altered(ctx, col, n, seed, p(b['altered'], ctypes.c_uint8), f0,
                                                                               p(b['i32'][0], i32), p(b['i32'][1], i32)),
        'pml_expected_counts': lambda: lib.pml_expected_counts(ctx, cb, ce, None, f0, None),
        'pml_loglik_gradient': lambda: lib.pml_loglik_gradient(ctx, cb, ce, f0, f1, p(b['i32'][0], i32)),
        'pml_expected_history': lambda: lib.pml_expected_history(ctx, cb, ce, f0, f1, f2),
        'pml_expected_history_eigen': lambda: lib.pml_expected_history_eigen(ctx, cb, ce, f0, f1, f2),
        'pml_history_through_time': lambda: lib.pml_history_through_time(ctx, cb, ce, node_time, boundaries, 1, f0, f1, f2),
        'pml_simulate_states': lambda: lib.pml_simulate_states(ctx, col, n, off, seed, states),
        'pml_sample_scenarios': lambda: lib.pml_sample_scenarios(ctx, col, n, off, seed, states, fallen),
        'pml_sample_histories': lambda: lib.pml_sample_histories(ctx, col, n, off, seed, states, f0, p(b['u32'][0], u32),
                                                                 p(b['u16'], ctypes.c_uint16), fallen),
        'pml_sample_histories_through_time': lambda: lib.pml_sample_histories_through_time(
            ctx, col, n, off, seed, node_time, boundaries, 1, states, f0, p(b['u32'][0], u32), p(b['u32'][1], u32), fallen),
    }
    status = calls[name]()
    return status, lib.pml_last_error().decode() if status != hip.PML_OK else ''


def _bad_column(call, names, column):
    """The cells of `column` (a bad column, in the state the context is in): a range that ends, or a column that lies, one past
    the last."""
    return {(name, column): call(name, ce=C + 1) if TABLE[name][column] == RANGE else call(name, col=C) for name in names}


@pytest.fixture(scope='module')
def observed():
    """{(entry, column): (status, message)}: both contexts walk from no model to a whole pass, every entry is called in every
    state that has a cell for it."""
    flat = synthetic.balanced_forest(LEVELS)
    assert len(flat.tips) == 8
    rng = np.random.default_rng(3)
    masks = np.stack([synthetic.one_hot_masks(flat, K, synthetic.tip_states(len(flat.tips), K, c)) for c in range(C)])
    models = {'f81': [(random_spec('F81', K, rng), (1.1, 0.0, 1.0)) for _ in range(C)],
              'eigen': [(random_spec('EIGEN', K, rng), (1.3, 0.0, 1.0)) for _ in range(C)]}
    b = _buffers(flat.n_nodes)
    seen = {}
    names = {kind: [name for name in TABLE if HOME[name] == kind] for kind in ('f81', 'eigen')}
    other = {'f81': 'eigen', 'eigen': 'f81'}
    with hip.Engine(flat, C, K) as f81, hip.Engine(flat, C, K) as eigen:
        engines = {'f81': f81, 'eigen': eigen}

        def call_on(kind):
            return lambda name, **args: _call(engines[kind]._lib, engines[kind]._ctx, name, b, **args)

        for kind in engines:
            for name in names[kind]:
                seen[name, 'no model'] = call_on(kind)(name)
        for kind, eng in engines.items():
            eng.set_models(models[kind])
            eng.set_masks(masks)
        for kind in engines:
            for name in names[kind]:
                seen[name, 'no pass'] = call_on(kind)(name)
            seen.update(_bad_column(call_on(kind), names[kind], 'no pass + bad column'))
            for name in names[other[kind]]:
                if 'wrong kind + no pass' in TABLE[name]:
                    seen[name, 'wrong kind + no pass'] = call_on(kind)(name)
        for kind, eng in engines.items():
            eng.bottom_up(is_marginal=True)
            for name in names[kind]:
                seen[name, 'bottom-up only'] = call_on(kind)(name)
        for kind, eng in engines.items():
            eng.marginal_pass(posterior=False, lh=False)
            seen.update(_bad_column(call_on(kind), names[kind], 'bad column'))
            for name in names[kind]:
                if 'n_repetitions = 0' in TABLE[name]:
                    seen[name, 'n_repetitions = 0'] = call_on(kind)(name, n=0)
                if 'rep_offset = -1' in TABLE[name]:
                    seen[name, 'rep_offset = -1'] = call_on(kind)(name, off=-1)
            for name in names[other[kind]]:
                if 'wrong kind' in TABLE[name]:
                    seen[name, 'wrong kind'] = call_on(kind)(name)
        # the refusals left both contexts answering
        for kind, eng in engines.items():
            assert np.isfinite(eng.expected_counts()).all()
    return seen


def test_the_table_is_whole(observed):
    assert len(TABLE) == 11
    assert all(column in COLUMNS for row in TABLE.values() for column in row)
    for column in COLUMNS:
        assert any(column in row for row in TABLE.values()), column
    assert set(observed) == {(name, column) for name, row in TABLE.items() for column in row}
    # the kinds: five entries of the F81 family, one of the eigen models
    assert sum('wrong kind' in row for row in TABLE.values()) == 6


@pytest.mark.parametrize('name', sorted(TABLE))
def test_row(name, observed):
    for column in COLUMNS:
        if column in TABLE[name]:
            print('{:36s} {:24s} {}'.format(name, column, observed[name, column]))
    for column, cell in TABLE[name].items():
        assert observed[name, column] == cell, (name, column)
