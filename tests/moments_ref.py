"""numpy restatement of the macroscopic state of include/bfsm.h (bfsm_moments_async, bfsm_maxwellian_async).

Grid v_a(i) = -L + (i + 1/2) * 2L/n_a on every axis, arrays [i][j][k], dV = dx dy dz.  A row per distribution:
    rho = dV sum f, m = dV sum v f, E = dV sum |v|^2 f, u = m / rho, T = (E / rho - |u|^2) / 3, H = dV sum_{f>0} f log f,
with u = T = 0 where rho == 0.  The six grid sums are exactly rounded (math.fsum).  Columns: RHO MX MY MZ E UX UY UZ T H.
"""
import math

import numpy as np

RHO, MX, MY, MZ, E, UX, UY, UZ, T, H = range(10)
COUNT = 10
EPS = np.finfo(np.float64).eps
SUM_COLUMNS = (RHO, MX, MY, MZ, E, H)       # the row columns the six grid sums land in


def axes(shape, L):
    return [-L + (np.arange(n) + 0.5) * (2.0 * L / n) for n in shape]


def cell_volume(shape, L):
    return float(np.prod([2.0 * L / n for n in shape]))


def terms(f, L):
    """[6, nx, ny, nz]: the summands f, vx f, vy f, vz f, |v|^2 f and f log f (0 where f <= 0) of one distribution."""
    vx, vy, vz = np.meshgrid(*axes(f.shape, L), indexing="ij")
    flogf = np.zeros_like(f)
    pos = f > 0
    flogf[pos] = f[pos] * np.log(f[pos])
    return np.stack([f, vx * f, vy * f, vz * f, (vx * vx + vy * vy + vz * vz) * f, flogf])


def sum_scales(f, L):
    """dV sum |psi_k f| for the six sums (|f log f| for H): what their rounding errors are measured against."""
    return cell_volume(f.shape, L) * np.abs(terms(f, L)).reshape(6, -1).sum(axis=1)


def moments(f, L):
    """The row(s) of f: [..., nx, ny, nz] -> [..., COUNT]."""
    if f.ndim > 3:
        return np.stack([moments(m, L) for m in f])
    dV = cell_volume(f.shape, L)
    s = [dV * math.fsum(t.ravel().tolist()) for t in terms(np.asarray(f, dtype=np.float64), L)]
    rho, m, e = s[0], np.array(s[1:4]), s[4]
    u, temp = np.zeros(3), 0.0
    if rho != 0.0:
        u = m / rho
        temp = (e / rho - float(u @ u)) / 3.0
    return np.array([rho, *m, e, *u, temp, s[5]])


def maxwellian(row, shape, L):
    """rho (2 pi T)^(-3/2) exp(-|v - u|^2 / 2T) on the grid from one row; 0 where rho or T is not finite and positive."""
    rho, temp = row[RHO], row[T]
    if not (np.isfinite(rho) and np.isfinite(temp) and rho > 0 and temp > 0):
        return np.zeros(shape)
    vx, vy, vz = np.meshgrid(*axes(shape, L), indexing="ij")
    d2 = (vx - row[UX]) ** 2 + (vy - row[UY]) ** 2 + (vz - row[UZ]) ** 2
    return rho / (2 * np.pi * temp) ** 1.5 * np.exp(-d2 / (2 * temp))


def assert_row(got, f, L, what=""):
    """`got` is the row of f within the derived tolerances: a pairwise / tree sum of n fp64 terms errs by at most about
    (log2 n + a few) eps sum |term|, so each of the six sums within 64 eps dV sum |psi_k f|; u within 1e-13 dV sum |v_a| |f| / |rho|
    per component and T within 1e-13 dV sum |v|^2 |f| / |rho| (the quotients of sums already that close)."""
    want = moments(f, L)
    sc = sum_scales(f, L)
    figures = []
    for k, col in enumerate(SUM_COLUMNS):
        figures.append((col, abs(got[col] - want[col]), 64 * EPS * sc[k]))
    if want[RHO] != 0.0:
        dV = cell_volume(f.shape, L)
        vabs = [np.abs(v) for v in np.meshgrid(*axes(f.shape, L), indexing="ij")]
        for a in range(3):
            figures.append((UX + a, abs(got[UX + a] - want[UX + a]), 1e-13 * dV * float((vabs[a] * np.abs(f)).sum()) / abs(want[RHO])))
        figures.append((T, abs(got[T] - want[T]), 1e-13 * sc[4] / abs(want[RHO])))
    else:
        figures += [(c, abs(got[c]), 0.0) for c in (UX, UY, UZ, T)]
    for col, err, tol in figures:
        assert err <= tol, (what, "column", col, "error", err, "tolerance", tol)
    return want


def assert_maxwellian(got, row, L, what=""):
    """`got` is the Maxwellian of `row` (the row the code under test produced itself): exp(-x) errs by about x eps e^-x <= eps / e
    in absolute terms and the prefactor by a few eps, so within 64 eps max M."""
    want = maxwellian(row, got.shape, L)
    err = float(np.abs(got - want).max())
    assert err <= 64 * EPS * float(want.max()), (what, err, float(want.max()))
