"""
acr(..., resolve_polytomies=True) on the GPU against the reference's run on the same forest and table
(tests/golden/polytomies.npz, part ``acr_``, tests/golden/make_golden_polytomies.py): five characters in one call
(F81 MPPA fixed, JC MAP optimised, EFT JOINT fixed, DOWNPASS, COPY); the final topology, the selected states of every
node in every result column, the posteriors and the result scalars.  Also: a binary forest gives the same bits with
and without resolution, and the pipeline writes the new nodes into its tables and named tree.
"""
import os

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN
from pastml_amd.tree import FlatForest, IS_POLYTOMY, read_tree

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN, 'polytomies.npz'))
COLUMNS = ['f81', 'jc', 'eft', 'mp', 'cp']


def _forest():
    n_tips, seed, max_arity, n_trees = (int(x) for x in G['acr_forest'])
    flat = FlatForest.random(n_tips, seed=seed, max_arity=max_arity, zero_frac=float(G['acr_zero_frac']),
                             n_trees=n_trees)
    return [flat.nodes[r] for r in flat.roots]


def _table():
    return pd.DataFrame({c: G['acr_table_' + c].tolist() for c in COLUMNS},
                        index=pd.Index(G['acr_table_names'].tolist(), name='id'))


def _parameters():
    f81 = G['acr_f81_params']
    states = G['acr_spec_f81'][2:].tolist()
    return {'f81': dict({'scaling_factor': float(f81[0])}, **{s: float(v) for s, v in zip(states, f81[1:])}),
            'eft': {'scaling_factor': float(G['acr_eft_sf'])}}


def _run(resolve_polytomies=True):
    from pastml_amd.acr import acr
    roots = _forest()
    results = acr(roots, _table(), prediction_method=[str(G['acr_spec_' + c][0]) for c in COLUMNS],
                  model=[str(G['acr_spec_' + c][1]) for c in COLUMNS], column2parameters=_parameters(),
                  resolve_polytomies=resolve_polytomies)
    return roots, results


def test_acr_resolve_polytomies_matches_reference():
    roots, results = _run()
    nodes = [n for r in roots for n in r.traverse()]
    names = [n.name for n in nodes]
    assert names == G['acr_names'].tolist()
    assert [n.up.name if n.up is not None else '' for n in nodes] == G['acr_parents'].tolist()
    np.testing.assert_allclose([n.dist for n in nodes], G['acr_dist'], rtol=0, atol=1e-15)
    assert [bool(getattr(n, IS_POLYTOMY, False)) for n in nodes] == G['acr_polytomy'].tolist()
    assert int(G['acr_polytomy'].sum()) == int(G['acr_created'][0]) - int(G['acr_removed'].sum()) > 0

    assert [r['character'] for r in results] == G['acr_result_characters'].tolist()
    fixed = {'f81', 'eft'}
    for r in results:
        c = r['character']
        states = G['acr_states_' + c].tolist()
        assert [str(s) for s in r['states']] == states
        s2i = {s: i for i, s in enumerate(states)}
        got = np.zeros((len(nodes), len(states)), dtype=np.int8)
        for i, n in enumerate(nodes):
            for s in getattr(n, c, set()):
                got[i, s2i[str(s)]] = 1
        mismatched = [names[i] for i in np.flatnonzero((got != G['acr_selected_' + c]).any(axis=1))]
        assert not mismatched, (c, mismatched[:10])
        if 'acr_marginal_' + c in G:
            table = r['marginal_probabilities']
            assert len(table) == len(nodes)
            np.testing.assert_allclose(table.loc[names, r['states']].to_numpy(dtype=np.float64), G['acr_marginal_' + c],
                                       rtol=0, atol=1e-9 if c in fixed else 1e-6)
        if 'acr_sf_' + c in G:
            np.testing.assert_allclose(float(r['model'].sf), float(G['acr_sf_' + c]), rtol=1e-6)
        prefix = 'acr_scalar_{}__'.format(c)
        for key in (k for k in G.files if k.startswith(prefix)):
            name = key[len(prefix):]
            assert name in r, (c, name)
            np.testing.assert_allclose(float(r[name]), float(G[key]), rtol=1e-8, err_msg='{} {}'.format(c, name))


def test_binary_forest_same_bits_with_and_without_resolution():
    from pastml_amd.acr import acr

    def run(resolve):
        flat = FlatForest.random(2000, seed=9, max_arity=2, zero_frac=0.05, n_trees=2)
        roots = [flat.nodes[r] for r in flat.roots]
        tips = [n for r in roots for n in r.traverse() if n.is_leaf()]
        rng = np.random.default_rng(4)
        df = pd.DataFrame({'loc': rng.choice(['a', 'b', 'c', 'd'], size=len(tips)),
                           'grp': rng.choice(['u', 'v'], size=len(tips))}, index=[t.name for t in tips])
        np.random.seed(17)
        res = acr(roots, df, prediction_method=['MPPA', 'DOWNPASS'], model='F81', resolve_polytomies=resolve)
        return roots, res

    roots0, res0 = run(False)
    roots1, res1 = run(True)
    assert [r.write() for r in roots0] == [r.write() for r in roots1]
    assert len(res0) == len(res1)
    for a, b in zip(res0, res1):
        assert sorted(a) == sorted(b)
        for key in a:
            if key == 'marginal_probabilities':
                assert a[key].equals(b[key])
            elif key == 'model':
                assert a[key].sf == b[key].sf and np.array_equal(a[key].frequencies, b[key].frequencies)
            elif isinstance(a[key], np.ndarray):
                assert np.array_equal(a[key], b[key])
            else:
                assert a[key] == b[key], key
    n0 = [n for r in roots0 for n in r.traverse()]
    n1 = [n for r in roots1 for n in r.traverse()]
    assert all(getattr(x, 'loc') == getattr(y, 'loc') and getattr(x, 'grp') == getattr(y, 'grp') for x, y in zip(n0, n1))


def test_pipeline_writes_polytomy_nodes(tmp_path):
    from pastml_amd.pipeline import pastml_pipeline
    roots = _forest()
    tree = tmp_path / 'forest.nwk'
    tree.write_text('\n'.join(r.write() for r in roots) + '\n')
    table = tmp_path / 'table.tab'
    _table()[['f81', 'mp']].to_csv(table, sep='\t')
    work = tmp_path / 'out'
    pastml_pipeline(str(tree), data=str(table), columns=['f81', 'mp'], prediction_method=['MPPA', 'DOWNPASS'],
                    model='F81', parameters={'f81': _parameters()['f81']}, work_dir=str(work), resolve_polytomies=True)
    files = sorted(os.listdir(work))
    assert 'combined_ancestral_states.tab' in files and 'named.tree_forest.nwk' in files
    assert 'params.character_f81.method_MPPA.model_F81.tab' in files
    assert 'marginal_probabilities.character_f81.model_F81.tab' in files
    combined = pd.read_csv(work / 'combined_ancestral_states.tab', sep='\t', dtype=str)
    polytomies = {n for n in combined['node'] if '.polytomy_' in n}
    assert polytomies
    marginal = pd.read_csv(work / 'marginal_probabilities.character_f81.model_F81.tab', sep='\t', index_col=0)
    assert polytomies <= set(marginal.index.map(str))
    named = (work / 'named.tree_forest.nwk').read_text().strip().split('\n')
    back = [read_tree(nwk) for nwk in named]
    back_names = {n.name for r in back for n in r.traverse()}
    assert back_names == set(combined['node'])
    assert polytomies <= back_names
    n_input = sum(1 for r in roots for _ in r.traverse())
    assert len(back_names) == n_input + len(polytomies)
