"""CPU tests of the conservative projection (include/bfsm.h: BFSM_FLAG_CONSERVE, bfsm_conserve_async).

The kernel bodies and the Conserver host code of csrc/bfsm_conserve.hpp run under the host lock-step emulator
(tests/emu/bfsm_emu_conserve.cpp, built into its own library with the flags of tests/emu/Makefile) and are compared with the
numpy restatement tests/conserve_ref.py: both forms (one launch per member, moments + apply), cubic and non-cubic boxes, a
size whose pair count is no multiple of the workgroup's stride, batches, and after the emulated full pipeline.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import conserve_ref as CR
import emu_lib as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd")
L_BOX = 11.0

_LIB = None


def _emu_flags():
    """CXX flags of tests/emu/Makefile's library rule (MFMA and EMUDEFS expanded the way make does)."""
    mk = open(os.path.join(HERE, "emu", "Makefile")).read()
    defs = re.search(r"^EMUDEFS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    mfma = []
    try:
        if re.search(r"\bfma\b", open("/proc/cpuinfo").read()):
            mfma = ["-mfma"]
    except OSError:
        pass
    return ["-O2"] + mfma + ["-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"] + defs


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "bfsm_emu_conserve.cpp")
        so = os.path.join(HERE, "emu", "libbfsm_emu_conserve.so")
        deps = [src, os.path.join(HERE, "emu", "bfsm_emu.cpp"), os.path.join(ROOT, "include", "bfsm.h")] + \
               [os.path.join(PKG, "csrc", n) for n in ("bfsm_core.hpp", "bfsm_pipeline.hpp", "bfsm_generic.hpp", "bfsm_conserve.hpp", "bfsm_calls.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            tmp = so[:-3] + ".%d.tmp.so" % os.getpid()
            subprocess.check_call([os.environ.get("CXX", "g++")] + _emu_flags() + ["-o", tmp, src])
            os.replace(tmp, so)
        from bfsm import capi
        L = ctypes.CDLL(so)
        L.bfsm_emu_conserve.argtypes = [ctypes.POINTER(capi.Desc), ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int)]
        L.bfsm_emu_conserve.restype = ctypes.c_int
        _LIB = L
    return _LIB


def emu_conserve(Q, L=L_BOX, form=-1, max_batch=0):
    """Q: [nx, ny, nz] or [nb, nx, ny, nz].  Returns (PQ, W, one-launch form used)."""
    shape = Q.shape[-3:]
    nb = Q.shape[0] if Q.ndim == 4 else 1
    one = np.ones(2)
    d, keep = E.make_desc(shape, (one, one), (one, one, one, one), 0.0, 1.0, L, max_batch=max(max_batch, nb))
    out = np.ascontiguousarray(Q, dtype=np.float64).copy()
    info = (ctypes.c_int * 2)()
    rc = lib().bfsm_emu_conserve(ctypes.byref(d), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nb, form, info)
    if rc:
        raise RuntimeError(f"bfsm_emu_conserve rc={rc}")
    return out, info[0], bool(info[1])


def _defect(shape, seed):
    """A smooth field plus a large defect in every invariant, so that lambda is far from zero."""
    rng = np.random.default_rng(seed)
    psi = CR.invariants(shape, L_BOX)
    return rng.standard_normal(shape) + np.einsum("k,kijl->ijl", rng.standard_normal(5) * [3, 0.5, -0.4, 0.3, 0.05], psi)


SHAPES = [(16, 16, 16), (12, 8, 20), (160, 4, 6), (4, 14, 160), (10, 6, 14), (18, 10, 26)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("form", [0, 1])
def test_both_forms_match_numpy(shape, form):
    Q = _defect(shape, sum(shape))
    got, W, small = emu_conserve(Q, form=form)
    assert small == (form == 1)
    want = CR.project(Q, L_BOX)
    assert np.abs(got - want).max() <= 1e-14 * np.abs(Q).max()
    assert np.all(np.abs(CR.moments(got, L_BOX)) <= 1e-13 * CR.moment_scale(Q, L_BOX))


def test_strides_and_form_choice():
    # 10 x 6 x 14: 420 pairs, no multiple of the 256-thread stride; 18 x 10 x 26: 2340 pairs over two workgroups
    assert emu_conserve(_defect((10, 6, 14), 1))[1:] == (1, True)
    assert emu_conserve(_defect((18, 10, 26), 1))[1:] == (2, False)
    assert emu_conserve(_defect((16, 16, 16), 1))[2] is True          # G = 16^3: the one-launch form


@pytest.mark.parametrize("form", [0, 1])
def test_batch_members_of_different_defects(form):
    shape = (18, 10, 26)
    Qs = np.stack([_defect(shape, 10 + i) * (1 + 4 * i) for i in range(3)])
    got, _, _ = emu_conserve(Qs, form=form, max_batch=4)
    for i in range(3):
        single, _, _ = emu_conserve(Qs[i], form=form)
        assert np.array_equal(got[i], single)                           # member i is bitwise the single projection
        assert np.abs(got[i] - CR.project(Qs[i], L_BOX)).max() <= 1e-14 * np.abs(Qs[i]).max()


def test_already_conserved_input_is_unchanged():
    P = CR.project(_defect((12, 8, 20), 5), L_BOX)
    for form in (0, 1):
        got, _, _ = emu_conserve(P, form=form)
        assert np.abs(got - P).max() <= 1e-15 * np.abs(P).max() * 10


@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 8, 20)])
def test_after_the_emulated_pipeline(oracle, shape):
    """The emulated collision (fused cube / size-generic box) followed by the emulated projection equals the numpy
    projection of the oracle Q."""
    import bfsm
    c = bfsm.reference_constants()
    if shape[0] == shape[1] == shape[2]:
        f = bfsm.perturbed_input(bfsm.bkw_solution(shape[0])[0])
    else:
        f = np.random.default_rng(1).random(shape) + 0.1
    gl = oracle.gauss_legendre(2, 0.0, c["R"])
    sph = oracle.spherical_design(6)
    Q, _ = E.collide(f, gl, sph, c["gamma"], c["b_gamma"], c["L"])
    got, _, _ = emu_conserve(Q, L=c["L"])
    ref = oracle.collide(f, gl, sph, c["gamma"], c["b_gamma"], c["L"])
    want = CR.project(ref, c["L"])
    assert np.abs(got - want).max() <= 1e-12 * np.abs(ref).max()
    assert np.all(np.abs(CR.moments(got, c["L"])) <= 1e-13 * CR.moment_scale(Q, c["L"]))
    assert np.abs(CR.moments(Q, c["L"])[[0, 4]]).max() > 1e-8 * CR.moment_scale(Q, c["L"]).max()   # unprojected: a defect
