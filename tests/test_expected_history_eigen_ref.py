"""
The restatements of tests/expected_history_eigen_ref.py against each other and against tests/expected_history_ref.py (host only).

An F81 model handed over as an eigen model (every non-zero eigenvalue equal: the fully degenerate case of Phi) has to give what
the F81 family's closed form gives, to 1e-12 of the largest entry: what is left is the rounding of A and Ainv, which is part of the
model for the eigen restatement and absent from the F81 one.  The float64 restatement, with the device's switch on |z|, has to
agree with the decimal one to 1e-11.  The identities hold on the decimal result to 1e-12 of their gross: they are exact where
A Ainv is exactly 1, and the given doubles miss that by a few 2^-53.
"""
import functools

import numpy as np
import pytest

import eigen_shape_cases as shapes
import expected_history_eigen_ref as eref
import expected_history_ref as href
import loglik_gradient_cases as cases

F81_VS_EIGEN = 1e-12
FLOAT64 = 1e-11
IDENTITY = 1e-12
KS = (2, 4, 7)


@functools.lru_cache(maxsize=None)
def _f81_case(k, shape):
    i = KS.index(k)
    flat = cases.forest(shape, seed=i)
    masks = cases.masks(flat, k, i)
    pi = cases.frequencies('F81', k, i)
    rates = cases.rates(i, 0.011 if shape != 'zeros' else 0.0)
    return flat, masks, pi, rates, eref.history(flat, masks, eref.f81_as_eigen(pi), *rates)


def _worst(values, h, k):
    return max(eref.scaled_errors(values['times'], h['times']).max(),
               eref.scaled_errors(values['branch_jumps'], h['branch_jumps']).max(),
               eref.scaled_errors(np.asarray(values['jumps']).ravel(), [x for i in range(k) for x in h['jumps'][i]]).max())


@pytest.mark.parametrize('shape', cases.SHAPES)
@pytest.mark.parametrize('k', KS)
def test_f81_as_eigen_model_gives_the_f81_closed_form(k, shape):
    flat, masks, pi, rates, h = _f81_case(k, shape)
    f81 = href.history(flat, masks, pi, *rates)
    got = dict(times=[float(x) for x in h['times']], branch_jumps=[float(x) for x in h['branch_jumps']],
               jumps=[[float(x) for x in h['jumps'][i]] for i in range(k)])
    worst = _worst(got, f81, k)
    print('F81 as eigen k={} {}: {:.3g}'.format(k, shape, worst))
    assert worst <= F81_VS_EIGEN
    assert abs(float(h['loglik'] - f81['loglik'])) <= 1e-12 * abs(float(f81['loglik']))
    if shape == 'zeros':
        zero = (flat.parent >= 0) & (flat.dist == 0)
        assert zero.any() and all(h['branch_jumps'][n] == 0 for n in np.flatnonzero(zero))


@pytest.mark.parametrize('shape', cases.SHAPES)
@pytest.mark.parametrize('k', KS)
def test_float64_restatement_on_the_degenerate_cases(k, shape):
    flat, masks, pi, rates, h = _f81_case(k, shape)
    v, q = eref.float_vectors(h)
    got = eref.history_float64(flat, eref.f81_as_eigen(pi), *rates, v=v, q=q)
    worst = _worst(got, h, k)
    print('float64 F81 as eigen k={} {}: {:.3g}'.format(k, shape, worst))
    assert worst <= FLOAT64


@pytest.mark.parametrize('k', [5, 20])
def test_float64_restatement_on_the_eigen_shapes(k):
    b = shapes.build(k, 'S')
    for c in range(2):
        h = eref.history(b['flat'], b['masks'][c], b['specs'][c], *b['rates'][c])
        v, q = eref.float_vectors(h)
        got = eref.history_float64(b['flat'], b['specs'][c], *b['rates'][c], v=v, q=q)
        worst = _worst(got, h, k)
        print('float64 eigen k={} column {}: {:.3g}'.format(k, c, worst))
        assert worst <= FLOAT64
        # the posteriors are those of the marginal pass this is built next to
        want = shapes.exact_pass(k, 'S', c)['posterior']
        assert np.abs(q - want).max() <= 1e-14
        _identities(h, b['flat'])


def _identities(h, flat):
    for name, left, right, gross in href.identities(h, flat):
        assert abs(float(left - right)) <= IDENTITY * float(gross), (name, left, right)
    assert all(h['jumps'][i][i] == 0 for i in h['jumps'])
    assert all(h['branch_jumps'][n] == 0 for n in np.flatnonzero(flat.parent < 0))


@pytest.mark.parametrize('shape', cases.SHAPES)
@pytest.mark.parametrize('k', KS)
def test_identities_on_the_decimal_result(k, shape):
    flat, _, _, _, h = _f81_case(k, shape)
    _identities(h, flat)


def test_jump_rows_are_rows_of_the_full_result():
    flat, masks, pi, rates, h = _f81_case(7, 'ragged')
    part = eref.history(flat, masks, eref.f81_as_eigen(pi), *rates, jump_rows=[0, 5])
    assert sorted(part['jumps']) == [0, 5]
    assert part['jumps'][5] == h['jumps'][5] and part['times'] == h['times']


def test_phi_series_against_expm1():
    z = np.array([0.0, 1e-300, 1e-17, 1e-9, 1e-3, 0.1, 0.25, 0.4999999])
    with np.errstate(invalid='ignore'):
        want = np.where(z == 0, 1.0, np.expm1(z) / np.where(z == 0, 1.0, z))
    assert np.abs(eref.phi_series(z) / want - 1).max() <= 4e-16
