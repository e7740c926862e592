"""CPU tests of the gain / loss split (include/bfsm.h, bfsm_collide_split*, bfsm_loss_rate_async).

tests/split_ref.py restates the two terms in numpy from tests/bilinear_ref.py; it is pinned here against the oracle through
the identity Q = Qgain - f nu.  The kernel bodies and launch sequences of the split then run under the host lock-step emulator
(tests/emu/bfsm_emu_split.cpp, built into its own library with the flags of tests/emu/Makefile) and are compared with that
restatement: fused cubes in both precisions, the size-generic path, and at 16^3 the exact / Hermitian gain mode, direction
shards, a batch, the bilinear form and the loss-only call.  Bounds: the project's (tests/test_gpu_bilinear.py), fp64 1e-12 and
fp32 5e-6, each relative to max|ref| of the array compared.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bilinear_ref as BR
import emu_lib as E
import split_ref as SR
from test_emu_bilinear import _emu_flags, _fields

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd")
TOL64 = 1e-12
TOL32 = 5e-6
GAMMA, B_GAMMA, L_BOX = 0.5, 0.3, 11.0
GL = (np.array([2.5, 7.0]), np.array([3.0, 2.0]))

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "bfsm_emu_split.cpp")
        so = os.path.join(HERE, "emu", "libbfsm_emu_split.so")
        deps = [src, os.path.join(HERE, "emu", "bfsm_emu.cpp"), os.path.join(ROOT, "include", "bfsm.h")] + \
               [os.path.join(PKG, "csrc", n) for n in ("bfsm_core.hpp", "bfsm_pipeline.hpp", "bfsm_generic.hpp", "bfsm_calls.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            tmp = so[:-3] + ".%d.tmp.so" % os.getpid()
            subprocess.check_call([os.environ.get("CXX", "g++")] + _emu_flags() + ["-o", tmp, src])
            os.replace(tmp, so)
        from bfsm import capi
        L = ctypes.CDLL(so)
        dp = ctypes.POINTER(ctypes.c_double)
        desc = ctypes.POINTER(capi.Desc)
        L.bfsm_emu_collide_split.argtypes = [desc, dp, dp, dp, ctypes.c_int, ctypes.c_int]
        L.bfsm_emu_collide_split.restype = ctypes.c_int
        L.bfsm_emu_collide_bilinear_split.argtypes = [desc, dp, dp, dp, dp, ctypes.c_int]
        L.bfsm_emu_collide_bilinear_split.restype = ctypes.c_int
        L.bfsm_emu_loss_rate.argtypes = [desc, dp, dp, ctypes.c_int]
        L.bfsm_emu_loss_rate.restype = ctypes.c_int
        _LIB = L
    return _LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _desc(shape, gl, sph, prec, dir_range=(0, 0), flags=0, max_batch=0):
    nv = shape[0] if shape[0] == shape[1] == shape[2] else shape
    return E.make_desc(nv, gl, sph, GAMMA, B_GAMMA, L_BOX, prec, dir_range, 0, flags, max_batch)


def emu_split(fs, gl, sph, prec=64, dir_range=(0, 0), with_loss=True, flags=0, max_batch=0):
    """fs: one distribution [nx][ny][nz] or a batch [nb][nx][ny][nz].  Returns (Qgain, nu); nu is None (a NULL pointer is
    passed) without the loss term."""
    fs = np.ascontiguousarray(fs, dtype=np.float64)
    nb = 1 if fs.ndim == 3 else fs.shape[0]
    d, keep = _desc(fs.shape[-3:], gl, sph, prec, dir_range, flags, max_batch or nb)
    Qg = np.full_like(fs, np.nan)
    nu = np.full_like(fs, np.nan) if with_loss else None
    rc = lib().bfsm_emu_collide_split(ctypes.byref(d), _p(fs), _p(Qg), _p(nu), nb, 1 if with_loss else 0)
    if rc:
        raise RuntimeError(f"bfsm_emu_collide_split rc={rc}")
    return Qg, nu


def emu_bilinear_split(g, f, gl, sph, prec=64, flags=0):
    g, f = (np.ascontiguousarray(a, dtype=np.float64) for a in (g, f))
    d, keep = _desc(f.shape, gl, sph, prec, flags=flags)
    Qg, nu = np.full_like(f, np.nan), np.full_like(f, np.nan)
    rc = lib().bfsm_emu_collide_bilinear_split(ctypes.byref(d), _p(g), _p(f), _p(Qg), _p(nu), 1)
    if rc:
        raise RuntimeError(f"bfsm_emu_collide_bilinear_split rc={rc}")
    return Qg, nu


def emu_loss_rate(fs, gl, sph, prec=64, dir_range=(0, 0)):
    fs = np.ascontiguousarray(fs, dtype=np.float64)
    nb = 1 if fs.ndim == 3 else fs.shape[0]
    d, keep = _desc(fs.shape[-3:], gl, sph, prec, dir_range, max_batch=nb)
    nu = np.full_like(fs, np.nan)
    rc = lib().bfsm_emu_loss_rate(ctypes.byref(d), _p(fs), _p(nu), nb)
    if rc:
        raise RuntimeError(f"bfsm_emu_loss_rate rc={rc}")
    return nu


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _tol(prec):
    return TOL64 if prec == 64 else TOL32


# ---- the numpy restatement against the oracle -------------------------------------------------------------------

def test_reference_assembles_to_the_oracle(oracle):
    """Qgain_ref - f nu_ref = the oracle's Q(f,f) at 16^3: fp64 numpy against the C oracle, the bound of
    test_emu_bilinear.py's pin of the same module."""
    _, f = _fields((16, 16, 16))
    gl = oracle.gauss_legendre(2, 0.0, 10.0)
    for sph in (BR.random_rule(7), oracle.spherical_design(6)):
        Qg, nu = SR.split(f, f, gl, sph, GAMMA, B_GAMMA, L_BOX)
        Qo = oracle.collide(f, gl, sph, GAMMA, B_GAMMA, L_BOX)
        assert float(np.abs(Qg - f * nu - Qo).max() / np.abs(Qo).max()) <= 1e-13


# ---- the emulated kernels against the restatement ---------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", [(16, 16, 16), (24, 24, 24), (32, 32, 32), (12, 8, 20)])
def test_split_matches_reference(shape, prec):
    _, f = _fields(shape, seed=sum(shape))
    sph = BR.random_rule(3, seed=sum(shape))
    Qg, nu = emu_split(f, GL, sph, prec)
    Qg_ref, nu_ref = SR.split(f, f, GL, sph, GAMMA, B_GAMMA, L_BOX)
    eg, en = _rel(Qg, Qg_ref), _rel(nu, nu_ref)
    print(f"{shape} fp{prec}: Qgain {eg:.2e}, nu {en:.2e}")
    # a kernel that still multiplied by f or still subtracted would be far outside the bound
    assert _rel(f * nu_ref, nu_ref) >= 1000 * _tol(prec) and _rel(Qg_ref - f * nu_ref, Qg_ref) >= 1000 * _tol(prec)
    assert eg <= _tol(prec) and en <= _tol(prec)


def test_exact_hermitian_handle(oracle):
    """Split is independent of the gain mode: EXACT_REDUCTIONS | HERMITIAN on an antipodal design."""
    _, f = _fields((16, 16, 16), seed=4)
    sph = oracle.spherical_design(12)
    Qg, nu = emu_split(f, GL, sph, flags=2 | 4)
    Qg_ref, nu_ref = SR.split(f, f, GL, sph, GAMMA, B_GAMMA, L_BOX)
    assert _rel(Qg, Qg_ref) <= TOL64 and _rel(nu, nu_ref) <= TOL64


def test_two_shards_sum_and_null_nu():
    _, f = _fields((16, 16, 16), seed=9)
    sph = BR.random_rule(3, seed=4)
    Q0, nu0 = emu_split(f, GL, sph, dir_range=(0, 2), with_loss=True)
    Q1, nu1 = emu_split(f, GL, sph, dir_range=(2, 6), with_loss=False)      # nu = NULL
    assert nu1 is None
    Qg_ref, nu_ref = SR.split(f, f, GL, sph, GAMMA, B_GAMMA, L_BOX)
    assert _rel(Q0 + Q1, Qg_ref) <= TOL64 and _rel(nu0, nu_ref) <= TOL64
    assert _rel(Q1, SR.split(f, f, GL, sph, GAMMA, B_GAMMA, L_BOX, dir_range=(2, 6))[0]) <= TOL64


def test_batch_members_are_the_single_calls():
    rng = np.random.default_rng(5)
    fs = rng.random((3, 16, 16, 16)) + 0.1
    sph = BR.random_rule(3, seed=1)
    Qg, nu = emu_split(fs, GL, sph)
    for i in range(3):
        Qi, nui = emu_split(fs[i], GL, sph, max_batch=3)          # a single call on the same (batch) handle
        assert np.array_equal(Qg[i], Qi) and np.array_equal(nu[i], nui), i
        Qg_ref, nu_ref = SR.split(fs[i], fs[i], GL, sph, GAMMA, B_GAMMA, L_BOX)
        assert _rel(Qg[i], Qg_ref) <= TOL64 and _rel(nu[i], nu_ref) <= TOL64


@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 8, 20)])
def test_bilinear_split(shape):
    g, f = _fields(shape, seed=11)
    sph = BR.random_rule(3, seed=5)
    Qg, nu = emu_bilinear_split(g, f, GL, sph)
    Qg_ref, nu_ref = SR.split(g, f, GL, sph, GAMMA, B_GAMMA, L_BOX)
    assert _rel(SR.split(f, g, GL, sph, GAMMA, B_GAMMA, L_BOX)[0], Qg_ref) >= 1000 * TOL64      # g and f exchanged would show
    assert _rel(Qg, Qg_ref) <= TOL64 and _rel(nu, nu_ref) <= TOL64


def test_bilinear_split_refuses_exact_reductions():
    g, f = _fields((16, 16, 16))
    with pytest.raises(RuntimeError, match="rc=2"):
        emu_bilinear_split(g, f, GL, BR.random_rule(4), flags=2)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 8, 20)])
def test_loss_only(shape, prec):
    rng = np.random.default_rng(sum(shape))
    fs = rng.random((2,) + shape) + 0.1
    sph = BR.random_rule(3)
    nu = emu_loss_rate(fs, GL, sph, prec)
    nu_shard = emu_loss_rate(fs[0], GL, sph, prec, dir_range=(1, 2))     # the loss does not depend on the shard
    for i in range(2):
        assert _rel(nu[i], BR.loss_rate(fs[i], GL, GAMMA, B_GAMMA, L_BOX)) <= _tol(prec)
    assert _rel(nu_shard, BR.loss_rate(fs[0], GL, GAMMA, B_GAMMA, L_BOX)) <= _tol(prec)


# ---- the C-ABI without a GPU ------------------------------------------------------------------------------------

def test_null_handle_is_invalid_without_gpu():
    so = os.path.join(PKG, "libbfsm_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", PKG, "-s", "libbfsm_hip.so"])
    from bfsm import capi
    L = capi.load_library()
    q = (ctypes.c_double * 8)()
    assert L.bfsm_collide_split(None, q, q, q) == 1   # BFSM_ERR_INVALID
    assert L.bfsm_collide_split_async(None, q, q, q, None) == 1
    assert L.bfsm_collide_split_batch_partial_async(None, q, q, q, 1, 1, None) == 1
    assert L.bfsm_collide_bilinear_split_partial_async(None, q, q, q, q, 1, None) == 1
    assert L.bfsm_loss_rate_async(None, q, q, 1, None) == 1
