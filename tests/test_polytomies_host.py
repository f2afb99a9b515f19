"""
Polytomy resolution on the host (pastml_amd.tree.resolve_trees / unresolve_trees, pastml/tree.py:344-492) against the
reference's own functions run on the same forest with the same prescribed predictions (tests/golden/polytomies.npz,
part ``edit_``, tests/golden/make_golden_polytomies.py), and the refusal of acr(resolve_polytomies=True) under a
multi-process launch.  No GPU.
"""
import os
import socket
import sys

import numpy as np
import torch.multiprocessing as mp

from conftest import GOLDEN, REPO
from pastml_amd.tree import FlatForest, IS_POLYTOMY, resolve_trees, unresolve_trees, get_flat_forest, StateSetColumn

G = np.load(os.path.join(GOLDEN, 'polytomies.npz'))
EDIT_STATES = {'a': ['0', '1', '2'], 'b': ['0', '1'], 'c': ['0', '1', '2', '3']}


def _forest(spec, zero_frac):
    n_tips, seed, max_arity, n_trees = (int(x) for x in spec)
    flat = FlatForest.random(n_tips, seed=seed, max_arity=max_arity, zero_frac=float(zero_frac), n_trees=n_trees)
    return [flat.nodes[r] for r in flat.roots]


def _nodes(roots):
    return [n for r in roots for n in r.traverse()]


def _prescribe(nodes, prefix):
    for c, states in EDIT_STATES.items():
        bits = G['{}sets_{}'.format(prefix, c)]
        assert bits.shape == (len(nodes), len(states))
        for n, row in zip(nodes, bits):
            if row.any():
                n.add_feature(c, {states[j] for j in np.flatnonzero(row)})
            elif c in n.features:
                n.del_feature(c)


def _check_topology(roots, prefix):
    nodes = _nodes(roots)
    assert [n.name for n in nodes] == G[prefix + 'names'].tolist()
    assert [n.up.name if n.up is not None else '' for n in nodes] == G[prefix + 'parents'].tolist()
    np.testing.assert_allclose([n.dist for n in nodes], G[prefix + 'dist'], rtol=0, atol=1e-15)
    assert [bool(getattr(n, IS_POLYTOMY, False)) for n in nodes] == G[prefix + 'polytomy'].tolist()
    # the cached flat forest follows the edits
    flat = get_flat_forest(roots)
    assert flat.n_nodes == len(nodes) and {id(n) for n in flat.nodes} == {id(n) for n in nodes}


def test_resolve_and_unresolve_match_reference():
    roots = _forest(G['edit_forest'], G['edit_zero_frac'])
    _prescribe(_nodes(roots), 'edit_resolve_')
    column2states = {c: np.array(s) for c, s in EDIT_STATES.items()}
    assert resolve_trees(column2states, roots) == int(G['edit_created'])
    _check_topology(roots, 'edit_resolved_')
    _prescribe(_nodes(roots), 'edit_unresolve_')
    assert unresolve_trees(column2states, roots) == int(G['edit_removed'])
    _check_topology(roots, 'edit_unresolved_')


def test_columnar_predictions_move_with_the_edit():
    """Predictions held in columns: new nodes take their closest child's, other nodes keep their own."""
    roots = _forest(G['edit_forest'], G['edit_zero_frac'])
    flat = get_flat_forest(roots)
    states = np.array(['0', '1', '2'])
    rng = np.random.default_rng(3)
    words = (np.uint64(1) << rng.integers(0, 3, size=flat.n_nodes).astype(np.uint64)).reshape(-1, 1)
    flat.set_column('a', StateSetColumn(words, states))
    before = {n.name: (n.a, n.dist) for n in flat.nodes}
    created = resolve_trees({'a': states}, roots)
    assert created > 0
    new = get_flat_forest(roots)
    assert new is not flat and new.n_nodes == flat.n_nodes + created
    assert isinstance(new.columns['a'], StateSetColumn) and new.columns['a'].absent is None
    n_polytomies = 0
    for n in new.nodes:
        if getattr(n, IS_POLYTOMY, False):
            n_polytomies += 1
            assert all(c.a == n.a for c in n.children) and n.a.isdisjoint(n.up.a)
            assert min(before[c.name][1] for c in n.children) == n.dist
        else:
            assert n.a == before[n.name][0]
    assert n_polytomies == created


def test_binary_forest_is_left_untouched():
    roots = _forest([300, 2, 2, 2], 0.0)
    flat = get_flat_forest(roots)
    states = np.array(['x', 'y'])
    for i, n in enumerate(flat.nodes):
        n.add_feature('s', {states[i % 2]})
    newick = [r.write() for r in roots]
    assert resolve_trees({'s': states}, roots) == 0
    assert unresolve_trees({'s': states}, roots) == 0
    assert [r.write() for r in roots] == newick
    assert get_flat_forest(roots) is flat


def test_named_polytomy_nodes_are_marked():
    from pastml_amd.tree import read_tree, name_tree
    tree = read_tree('((a:1,b:1)r.polytomy_0:0.5,c:1,d:1);')
    name_tree(tree)
    assert [n.name for n in tree.traverse() if getattr(n, IS_POLYTOMY, False)] == ['r.polytomy_0']


# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _refusing_rank(rank, world, port, out):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      PASTML_AMD_COMM='gloo')
    from pastml_amd import sharding
    from pastml_amd.acr import acr
    from pastml_amd.tree import read_tree
    comm = sharding.init()
    try:
        tree = read_tree('((a:1,b:1,c:1):1,(d:1,e:1):1);')
        for n, v in zip(tree, 'xxyyx'):
            n.add_feature('loc', {v})
        try:
            acr(tree, columns=['loc'], column2states={'loc': np.array(['x', 'y'])}, resolve_polytomies=True)
            out.put((rank, None))
        except NotImplementedError as e:
            out.put((rank, str(e)))
        comm.barrier()
    finally:
        sharding.shutdown()


def test_acr_refuses_resolve_polytomies_with_several_ranks():
    ctx = mp.get_context('spawn')
    out = ctx.SimpleQueue()
    mp.start_processes(_refusing_rank, args=(2, _free_port(), out), nprocs=2, join=True, start_method='spawn')
    got = dict(out.get() for _ in range(2))
    assert sorted(got) == [0, 1]
    for message in got.values():
        assert message is not None and 'resolve_polytomies' in message and '2 ranks' in message
