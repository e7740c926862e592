"""numpy restatement of the bilinear collision operator Q(g,f) of include/bfsm.h (test infrastructure).

The oracle loop (oracle/bfsm_oracle.c, bfsm_oracle_collide_ex) with three changes: A1 is formed from g_hat = FFT(g),
A2 from f_hat = FFT(f) with the same phase factors, and the loss is multiplied by g:
    Q(g,f) = Re IFFT(Q_gain_hat) - g * Re IFFT(beta2 f_hat / G).
Q(f,f) is the oracle's operator; tests/test_emu_bilinear.py pins this module to the oracle with g = f.
"""
import numpy as np

_EPS = np.finfo(np.float64).eps


def _sincc(x):
    return np.sin(x + _EPS) / (x + _EPS)


def _modes(n):
    return np.concatenate([np.arange(0, n // 2), np.arange(-(n // 2), 0)]).astype(np.float64)


def _norm_l(shape):
    lx, ly, lz = np.meshgrid(_modes(shape[0]), _modes(shape[1]), _modes(shape[2]), indexing="ij")
    return lx, ly, lz, np.sqrt(lx * lx + ly * ly + lz * lz)


def beta2(shape, gl, gamma, b_gamma, L):
    rho, wr = gl
    norm_l = _norm_l(shape)[3]
    b2 = np.zeros(shape)
    for r in range(len(rho)):
        b2 += 16 * np.pi ** 2 * b_gamma * wr[r] * rho[r] ** (gamma + 2) * _sincc(np.pi * rho[r] * norm_l / L)
    return b2


def loss_rate(h, gl, gamma, b_gamma, L):
    """Lambda[h] = Re IFFT(beta2 h_hat / G): the loss term of Q(g,h) is g * Lambda[h]."""
    h = np.asarray(h, dtype=np.float64)
    return np.fft.ifftn(beta2(h.shape, gl, gamma, b_gamma, L) * np.fft.fftn(h)).real


def collide_bilinear(g, f, gl, sph, gamma, b_gamma, L, dir_range=None, with_loss=True):
    """Q(g,f) on the box of g (== that of f); dir_range = (b0, b1): the gain of that shard of directions only."""
    g = np.asarray(g, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    assert g.shape == f.shape
    G = f.size
    rho, wr = gl
    sx, sy, sz, ws = sph
    lx, ly, lz, norm_l = _norm_l(f.shape)
    g_hat, f_hat = np.fft.fftn(g), np.fft.fftn(f)
    qhat = np.zeros(f.shape, dtype=np.complex128)
    B = len(rho) * len(ws)
    b0, b1 = (0, B) if dir_range is None else dir_range
    for b in range(b0, b1):
        r, s = divmod(b, len(ws))
        tmp = -(np.pi / (2 * L)) * rho[r] * (lx * sx[s] + ly * sy[s] + lz * sz[s])
        a = np.cos(tmp) + 1j * np.sin(tmp)
        A1 = np.fft.ifftn(a * g_hat)
        A2 = np.fft.ifftn(np.conj(a) * f_hat)
        weight = (1.0 / G) * wr[r] * ws[s] * rho[r] ** (gamma + 2)
        qhat += weight * 4 * np.pi * b_gamma * _sincc(np.pi * rho[r] * norm_l / (2 * L)) * np.fft.fftn(A1 * A2)
    Q = (np.fft.ifftn(qhat) * G).real
    if with_loss:
        Q = Q - g * loss_rate(f, gl, gamma, b_gamma, L)
    return Q


def random_rule(n, seed=7):
    """A spherical rule WITHOUT antipodal symmetry: n random unit vectors, positive weights summing to 4 pi.
    With it the gain of Q(g,f) is not symmetric in (g,f), so the convention A1 <- g, A2 <- f is what is tested."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    w = rng.random(n) + 0.5
    w *= 4 * np.pi / w.sum()
    return v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy(), w
