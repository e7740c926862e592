"""numpy restatement of the conservative projection of include/bfsm.h (BFSM_FLAG_CONSERVE, bfsm_conserve_async).

Grid v_a(i) = -L + (i + 1/2) * 2L/n_a on every axis, arrays [i][j][k].  Basis psi = {1, vx, vy, vz, |v|^2 - c} with
c = mean of |v|^2 over the grid (orthogonal on the symmetric grid), and
    PQ = Q - sum_k (<psi_k, Q> / <psi_k, psi_k>) psi_k,   <a, b> = sum over the grid points.
tests/test_conserve_ref.py pins it against the explicit form Q - C^T (C C^T)^-1 C Q of Gamba & Tharkabhushanam.
"""
import numpy as np


def axes(shape, L):
    return [-L + (np.arange(n) + 0.5) * (2.0 * L / n) for n in shape]


def basis(shape, L):
    """[5, nx, ny, nz]: 1, vx, vy, vz, |v|^2 - c."""
    vx, vy, vz = np.meshgrid(*axes(shape, L), indexing="ij")
    v2 = vx * vx + vy * vy + vz * vz
    return np.stack([np.ones(shape), vx, vy, vz, v2 - v2.mean()])


def invariants(shape, L):
    """[5, nx, ny, nz]: 1, vx, vy, vz, |v|^2 (the rows of C)."""
    vx, vy, vz = np.meshgrid(*axes(shape, L), indexing="ij")
    return np.stack([np.ones(shape), vx, vy, vz, vx * vx + vy * vy + vz * vz])


def moments(Q, L):
    """<psi_k, Q> for the last three axes of Q: [..., 5]."""
    psi = basis(Q.shape[-3:], L)
    return np.einsum("kijl,...ijl->...k", psi, Q)


def moment_scale(Q, L):
    """sum_i |psi_k(v_i) Q_i|: the size the moments of Q are measured against, [..., 5]."""
    psi = basis(Q.shape[-3:], L)
    return np.einsum("kijl,...ijl->...k", np.abs(psi), np.abs(Q))


def project(Q, L):
    """PQ for an array [..., nx, ny, nz] (a batch projects member by member)."""
    psi = basis(Q.shape[-3:], L)
    lam = moments(Q, L) / np.einsum("kijl,kijl->k", psi, psi)
    return Q - np.einsum("...k,kijl->...ijl", lam, psi)


def project_explicit(Q, L):
    """Q - C^T (C C^T)^-1 C Q, C = rows {1, v, |v|^2} (Gamba & Tharkabhushanam's form), one array."""
    C = invariants(Q.shape, L).reshape(5, -1)
    q = Q.reshape(-1)
    return (q - C.T @ np.linalg.solve(C @ C.T, C @ q)).reshape(Q.shape)
