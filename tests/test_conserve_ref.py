"""CPU: the numpy restatement of the conservative projection (tests/conserve_ref.py) is the projection it claims to be."""
import numpy as np
import pytest

import conserve_ref as CR

SHAPES = [(16, 16, 16), (12, 8, 20), (160, 4, 6), (4, 14, 160), (10, 6, 14)]


def _q(shape, seed=1):
    return np.random.default_rng(seed).standard_normal(shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_moments_of_PQ_vanish(shape):
    Q = _q(shape)
    P = CR.project(Q, 7.5)
    assert np.all(np.abs(CR.moments(P, 7.5)) <= 1e-13 * CR.moment_scale(Q, 7.5))
    assert np.abs(CR.moments(Q, 7.5)).max() > 1e-3 * CR.moment_scale(Q, 7.5).max()     # the input is not conserved


@pytest.mark.parametrize("shape", SHAPES)
def test_projection_is_idempotent(shape):
    P = CR.project(_q(shape, 2), 11.0)
    assert np.abs(CR.project(P, 11.0) - P).max() <= 1e-14 * np.abs(P).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_basis_is_orthogonal(shape):
    psi = CR.basis(shape, 9.0).reshape(5, -1)
    gram = psi @ psi.T
    d = np.sqrt(np.diag(gram))
    off = gram / np.outer(d, d) - np.eye(5)
    assert np.abs(off).max() <= 1e-13


@pytest.mark.parametrize("shape", SHAPES)
def test_matches_the_explicit_form(shape):
    Q = _q(shape, 3)
    assert np.abs(CR.project(Q, 11.04) - CR.project_explicit(Q, 11.04)).max() <= 1e-13 * np.abs(Q).max()


def test_batch_projects_member_by_member():
    Qs = np.stack([_q((12, 8, 20), s) * (s + 1) for s in range(3)])
    P = CR.project(Qs, 5.0)
    for i in range(3):
        assert np.array_equal(P[i], CR.project(Qs[i], 5.0))
