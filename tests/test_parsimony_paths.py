"""
The switch between the host and the device path of the parsimonious methods (PASTML_AMD_PARSIMONY, pastml_amd.parsimony.choose_path)
and the C-ABI of the device path, as far as a box without a GPU can tell.
"""
import os
import re

import numpy as np
import pytest

from conftest import load_golden, GOLDEN
from pastml_amd import hip
from pastml_amd import parsimony as P
from pastml_amd.parsimony import STEPS, MP, DOWNPASS


def test_switch_parses(monkeypatch):
    monkeypatch.delenv(P.PATH_VARIABLE, raising=False)
    assert P.parsimony_path() == 'auto'
    for value, want in (('host', 'host'), ('DEVICE', 'device'), (' Auto ', 'auto'), ('', 'auto')):
        monkeypatch.setenv(P.PATH_VARIABLE, value)
        assert P.parsimony_path() == want
    monkeypatch.setenv(P.PATH_VARIABLE, 'gpu')
    with pytest.raises(ValueError, match=P.PATH_VARIABLE):
        P.parsimony_path()


def test_host_is_chosen_where_it_must_be(monkeypatch):
    states = [np.arange(4)]
    monkeypatch.setenv(P.PATH_VARIABLE, 'host')
    assert P.choose_path(10 ** 6, ['c'], states) == P.HOST
    monkeypatch.setenv(P.PATH_VARIABLE, 'auto')
    assert P.choose_path(100, ['c'], states) == P.HOST                       # too small a job
    assert P.choose_path(10 ** 6, ['c'], [np.arange(513)]) == P.HOST         # beyond the device path's bound
    monkeypatch.setattr(P, '_device_ready', lambda: False)
    assert P.choose_path(10 ** 6, ['c'], states) == P.HOST                   # no device
    monkeypatch.setattr(P, '_device_ready', lambda: True)
    assert P.choose_path(10 ** 6, ['c'], states) == P.DEVICE
    # the threshold is on nodes x characters x words, and lower where a context holds the tree already
    assert P.AUTO_MIN_WORK_WITH_CONTEXT <= P.AUTO_MIN_WORK
    n = P.AUTO_MIN_WORK_WITH_CONTEXT
    assert P.choose_path(n, ['c'], states, has_context=True) == P.DEVICE
    assert P.choose_path(n - 1, ['c'], states, has_context=True) == P.HOST
    assert P.choose_path((P.AUTO_MIN_WORK + 1) // 2, ['c', 'd'], [np.arange(70)] * 2) == P.DEVICE


def test_device_refuses_513_states_by_name(monkeypatch):
    monkeypatch.setenv(P.PATH_VARIABLE, 'device')
    with pytest.raises(ValueError, match='Character wide has 513 states'):
        P.choose_path(1000, ['narrow', 'wide'], [np.arange(3), np.arange(513)])


def test_device_without_a_device_raises(monkeypatch):
    if hip.device_count() > 0:
        monkeypatch.setattr(hip, 'device_count', lambda: 0)
    monkeypatch.setenv(P.PATH_VARIABLE, 'device')
    with pytest.raises(hip.HipUnavailableError):
        P.choose_path(1000, ['c'], [np.arange(3)])


def test_device_without_a_library_raises(monkeypatch):
    def missing():
        raise hip.HipUnavailableError('no library')
    monkeypatch.setattr(hip, 'load_library', missing)
    monkeypatch.setenv(P.PATH_VARIABLE, 'device')
    with pytest.raises(hip.HipUnavailableError):
        P.choose_path(1000, ['c'], [np.arange(3)])


def test_auto_without_a_device_takes_the_host_and_equals_the_reference(monkeypatch):
    import pandas as pd
    from pastml_amd.acr import acr
    from pastml_amd.tree import read_tree
    monkeypatch.setenv(P.PATH_VARIABLE, 'auto')
    monkeypatch.setattr(P, '_device_ready', lambda: False)
    monkeypatch.setattr(P, 'AUTO_MIN_WORK', 1)   # (large enough a job: only the missing device keeps it on the host)
    monkeypatch.setattr(P, 'parsimonious_acr_batch', lambda *a, **kw: pytest.fail('the device path was taken'))
    z = load_golden('parsimony')
    tree = read_tree(os.path.join(GOLDEN, 'data', 'Albanian.tree.152tax.tre'))
    df = pd.read_csv(os.path.join(GOLDEN, 'data', 'data.txt'), index_col=0, header=0)[['Country']]
    df['Again'] = df['Country']
    res = acr(tree, df, prediction_method=[MP, DOWNPASS])
    assert [(r['character'], r['method']) for r in res] == [('Country_ACCTRAN', 'ACCTRAN'), ('Country_DOWNPASS', 'DOWNPASS'),
                                                            ('Country_DELTRAN', 'DELTRAN'), ('Again', 'DOWNPASS')]
    for r in res[:3]:
        tag = 'alb_MP_{}_'.format(r['method'])
        assert r[STEPS] == int(z[tag + 'steps'])
        assert float(r['num_scenarios']) == float(z[tag + 'num_scenarios'])
        assert r['num_unresolved_nodes'] == int(z[tag + 'num_unresolved_nodes'])
    assert res[3][STEPS] == int(z['alb_DOWNPASS_DOWNPASS_steps'])


def test_acr_serves_its_parsimonious_characters_in_one_batch(monkeypatch):
    """acr() hands all of its 'mp' plan items to the batched form together (one device call per number of states)."""
    import pandas as pd
    from pastml_amd.acr import acr
    from pastml_amd.tree import read_tree
    seen = []

    def fake_batch(forest, characters, methods, states, num_nodes, num_tips, engine=None):
        seen.append((list(characters), list(methods)))
        return [P.parsimonious_acr(forest, c, m, s, num_nodes, num_tips) for c, m, s in zip(characters, methods, states)]

    monkeypatch.setenv(P.PATH_VARIABLE, 'auto')
    monkeypatch.setattr(P, '_device_ready', lambda: True)
    monkeypatch.setattr(P, 'AUTO_MIN_WORK', 1)
    monkeypatch.setattr(P, 'parsimonious_acr_batch', fake_batch)
    tree = read_tree(os.path.join(GOLDEN, 'data', 'Albanian.tree.152tax.tre'))
    df = pd.read_csv(os.path.join(GOLDEN, 'data', 'data.txt'), index_col=0, header=0)[['Country']]
    df['B'], df['C'] = df['Country'], df['Country']
    res = acr(tree, df, prediction_method=[MP, 'COPY', 'DELTRAN'])
    assert seen == [(['Country', 'C'], [MP, 'DELTRAN'])]
    assert [r['method'] for r in res] == ['ACCTRAN', 'DOWNPASS', 'DELTRAN', 'COPY', 'DELTRAN']


def test_header_exports_and_signatures_agree_on_the_entry():
    import ctypes
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, '..', 'include', 'pastml_hip.h')) as f:
        header = f.read()
    m = re.search(r'int pml_parsimony\(([^;]*)\);', header)
    assert m, 'pml_parsimony is not declared in pastml_hip.h'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    assert len(params) == len(hip.SIGNATURES['pml_parsimony']) == 8
    assert [('*' in p) for p in params] == [True, False, False, True, False, True, True, True]
    assert re.search(r'PML_PARS_ACCTRAN = 1, PML_PARS_DOWNPASS = 2, PML_PARS_DELTRAN = 4', header)
    assert (hip.PARS_ACCTRAN, hip.PARS_DOWNPASS, hip.PARS_DELTRAN) == (1, 2, 4)
    assert 'pml_parsimony_info' in hip.SIGNATURES
    lib = ctypes.CDLL(hip.library_path())
    assert hasattr(lib, 'pml_parsimony') and hasattr(lib, 'pml_parsimony_info')
    assert hip.MAX_STATES == P.MAX_DEVICE_STATES == 512
