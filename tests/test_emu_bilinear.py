"""CPU tests of the bilinear collision operator Q(g,f) (include/bfsm.h, bfsm_collide_bilinear*).

tests/bilinear_ref.py restates the definition in numpy; it is pinned here against the oracle (g = f and polarization).
The kernel bodies and launch sequences of the bilinear form then run under the host lock-step emulator
(tests/emu/bfsm_emu_bilinear.cpp, built into its own library with the flags of tests/emu/Makefile) and are compared with
that restatement on every route: the fused cubes (N = 16 on the plane-tile pipeline), the three sequences of the
size-generic path, direction shards, and g = f against the emulated Q(f,f).  The case table of the GPU suite's fused cubes
(tests/bilinear_cases.py) is checked against fused_grid() and the library's plan.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bilinear_cases as BC
import bilinear_ref as BR
import emu_lib as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd")
R = 10.0

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
        src = os.path.join(HERE, "emu", "bfsm_emu_bilinear.cpp")
        so = os.path.join(HERE, "emu", "libbfsm_emu_bilinear.so")
        deps = [src, os.path.join(HERE, "emu", "bfsm_emu.cpp"), os.path.join(ROOT, "include", "bfsm.h")] + \
               [os.path.join(PKG, "csrc", n) for n in ("bfsm_core.hpp", "bfsm_pipeline.hpp", "bfsm_generic.hpp", "bfsm_calls.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            tmp = so[:-3] + ".%d.tmp.so" % os.getpid()
            subprocess.check_call([os.environ.get("CXX", "g++")] + _emu_flags() + ["-o", tmp, src])
            os.replace(tmp, so)
        from bfsm import capi
        L = ctypes.CDLL(so)
        dp = ctypes.POINTER(ctypes.c_double)
        L.bfsm_emu_collide_bilinear.argtypes = [ctypes.POINTER(capi.Desc), dp, dp, dp, ctypes.c_int]
        L.bfsm_emu_collide_bilinear.restype = ctypes.c_int
        _LIB = L
    return _LIB


def emu_bilinear(g, f, gl, sph, gamma, b_gamma, L, precision=64, dir_range=(0, 0), with_loss=True, flags=0, same=False,
                 max_chunk=0):
    """same=True passes f's buffer as g (the g == f pointer case of the C-ABI)."""
    nv = f.shape[0] if f.shape[0] == f.shape[1] == f.shape[2] else f.shape
    d, keep = E.make_desc(nv, gl, sph, gamma, b_gamma, L, precision, dir_range, max_chunk, flags)
    f = np.ascontiguousarray(f, dtype=np.float64)
    g = f if same else np.ascontiguousarray(g, dtype=np.float64)
    Q = np.empty_like(f)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib().bfsm_emu_collide_bilinear(ctypes.byref(d), g.ctypes.data_as(dp), f.ctypes.data_as(dp), Q.ctypes.data_as(dp),
                                         1 if with_loss else 0)
    if rc:
        raise RuntimeError(f"bfsm_emu_collide_bilinear rc={rc}")
    return Q


def _fields(shape, seed=3):
    rng = np.random.default_rng(seed)
    f = rng.random(shape) + 0.1
    g = rng.random(shape) + 0.1
    return g, f


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- the numpy restatement against the oracle -------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(16, 16, 16), (24, 24, 24), (12, 8, 20)])
@pytest.mark.parametrize("gamma", [0.0, 1.0])
def test_reference_with_g_equal_f_is_the_oracle(oracle, shape, gamma):
    _, f = _fields(shape)
    gl = oracle.gauss_legendre(2, 0.0, R)
    L = 11.0
    for sph in (BR.random_rule(7), oracle.spherical_design(6)):
        Qo = oracle.collide(f, gl, sph, gamma, 0.3, L)
        assert _rel(BR.collide_bilinear(f, f, gl, sph, gamma, 0.3, L), Qo) <= 1e-13


@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 8, 20)])
def test_reference_polarization_against_the_oracle(oracle, shape):
    """Q(g,f) + Q(f,g) = Q(f+g) - Q(f) - Q(g), with a non-antipodal rule (the gain alone is not symmetric there)."""
    g, f = _fields(shape, seed=11)
    gl = oracle.gauss_legendre(2, 0.0, R)
    sph = BR.random_rule(7, seed=5)
    L = 11.0
    lhs = BR.collide_bilinear(g, f, gl, sph, 0.5, 0.3, L) + BR.collide_bilinear(f, g, gl, sph, 0.5, 0.3, L)
    rhs = oracle.collide(f + g, gl, sph, 0.5, 0.3, L) - oracle.collide(f, gl, sph, 0.5, 0.3, L) - \
        oracle.collide(g, gl, sph, 0.5, 0.3, L)
    assert _rel(lhs, rhs) <= 1e-12


def test_reference_is_not_symmetric_for_a_non_antipodal_rule(oracle):
    """The convention (A1 from g, A2 from f) matters for such a rule: otherwise the tests above could not tell them apart."""
    g, f = _fields((12, 8, 20), seed=2)
    gl = oracle.gauss_legendre(2, 0.0, R)
    sph = BR.random_rule(7)
    lam_f, lam_g = (BR.loss_rate(h, gl, 0.0, 0.3, 11.0) for h in (f, g))
    gain_gf = BR.collide_bilinear(g, f, gl, sph, 0.0, 0.3, 11.0) + g * lam_f
    gain_fg = BR.collide_bilinear(f, g, gl, sph, 0.0, 0.3, 11.0) + f * lam_g
    assert _rel(gain_gf, gain_fg) > 1e-6


# ---- the emulated kernels against the restatement ---------------------------------------------------------------

@pytest.mark.parametrize("nv,prec,tol,flags", [
    (16, 64, 1e-12, 0), (16, 64, 1e-12, 8),     # N = 16: the plane-tile pipeline, with or without BFSM_FLAG_NO_SMALL_PATH
    (24, 64, 1e-12, 0), (32, 64, 1e-12, 0), (48, 64, 1e-12, 0),
    (16, 32, 1e-4, 0), (24, 32, 1e-4, 0), (32, 32, 1e-4, 0), (48, 32, 1e-4, 0),
])
def test_fused_cubes_match_reference(oracle, nv, prec, tol, flags):
    f0, _, L, _ = oracle.bkw(nv)
    f = oracle.perturbed_input(f0)
    g = oracle.perturbed_input(f0 * (1.0 + 0.2 * np.linspace(-1, 1, nv)[:, None, None]), seed=0xB11)
    gl = oracle.gauss_legendre(2, 0.0, R)
    sph = BR.random_rule(6)
    Q = emu_bilinear(g, f, gl, sph, 0.0, 1.0 / (4 * np.pi), L, prec, flags=flags)
    ref = BR.collide_bilinear(g, f, gl, sph, 0.0, 1.0 / (4 * np.pi), L)
    assert _rel(Q, ref) <= tol


@pytest.mark.parametrize("nv,prec,n_gl,n_dir,max_chunk", [
    (40, 64, 1, 3, 0), (64, 64, 1, 3, 0), (80, 64, 1, 3, 0), (96, 64, 1, 3, 0),
    (40, 32, 1, 3, 0), (64, 32, 1, 3, 0), (80, 32, 1, 3, 0), (96, 32, 1, 3, 0),
    pytest.param(128, 64, 1, 3, 0, marks=pytest.mark.slow), pytest.param(128, 32, 1, 3, 0, marks=pytest.mark.slow),
    (64, 32, 2, 7, 2), (96, 64, 2, 7, 2),     # chunks of 2 directions, across the radial-node boundary at 7
])
def test_larger_fused_cubes_match_reference(nv, prec, n_gl, n_dir, max_chunk):
    """The fused cubes of test_fused_cubes_match_reference from N = 40 up, where KA re-reads planes, splits its exchange
    or interleaves its scratch (tests/bilinear_cases.py).  Inputs of their own: random g and f, a rule without antipodal
    symmetry and gamma != 0 (the cases above keep theirs and their bounds).  Bounds: the GPU suite's, 1e-12 in fp64 and
    5e-6 in fp32."""
    rng = np.random.default_rng(1)
    g = rng.random((nv, nv, nv)) + 0.1
    f = rng.random((nv, nv, nv)) + 0.1
    gl = (np.array([2.5, 7.0])[:n_gl], np.array([3.0, 2.0])[:n_gl])
    sph = BR.random_rule(n_dir, seed=nv)
    Q = emu_bilinear(g, f, gl, sph, 0.5, 0.3, 11.0, prec, max_chunk=max_chunk)
    ref = BR.collide_bilinear(g, f, gl, sph, 0.5, 0.3, 11.0)
    err = _rel(Q, ref)
    print(f"N={nv} fp{prec} {n_gl}x{n_dir} max_chunk={max_chunk}: max rel err {err:.2e}")
    assert err <= (1e-12 if prec == 64 else 5e-6)


@pytest.mark.parametrize("shape,prec,tol", [
    ((16, 8, 6), 64, 1e-12),      # fused sequence (plane-pair kernel in double precision)
    ((12, 6, 10), 32, 1e-4),      # fused sequence, single precision (one plane workgroup per sign)
    ((8, 14, 6), 64, 1e-12),      # x-line sequence behind per-axis passes (radix-7 y axis: no plane kernel)
    ((154, 4, 4), 64, 1e-12),     # per-axis sequence, x pass first (table-driven radices on x: no x-line kernel)
    ((14, 22, 26), 64, 1e-12),    # per-axis sequence without the plane kernel
    ((160, 4, 6), 64, 1e-12),     # long x lines: 8 lines per workgroup in the x-line kernel
    ((4, 14, 160), 64, 1e-12),    # ... in the z pass that forms the phase
])
def test_size_generic_sequences_match_reference(shape, prec, tol):
    g, f = _fields(shape, seed=sum(shape))
    gl = (np.array([2.5, 7.0]), np.array([3.0, 2.0]))
    sph = BR.random_rule(5, seed=sum(shape))
    Q = emu_bilinear(g, f, gl, sph, 0.5, 0.3, 11.0, prec)
    ref = BR.collide_bilinear(g, f, gl, sph, 0.5, 0.3, 11.0)
    assert _rel(Q, ref) <= tol


@pytest.mark.parametrize("shape", [(32, 32, 32), (16, 8, 6)])
def test_direction_shards_add_up(oracle, shape):
    g, f = _fields(shape, seed=9)
    gl = oracle.gauss_legendre(2, 0.0, R)
    sph = BR.random_rule(6, seed=4)
    B = 12
    Q0 = emu_bilinear(g, f, gl, sph, 0.0, 0.3, 11.0, dir_range=(0, 5), with_loss=True)
    Q1 = emu_bilinear(g, f, gl, sph, 0.0, 0.3, 11.0, dir_range=(5, B), with_loss=False)
    ref = BR.collide_bilinear(g, f, gl, sph, 0.0, 0.3, 11.0)
    assert _rel(Q0 + Q1, ref) <= 1e-12
    assert _rel(Q1, BR.collide_bilinear(g, f, gl, sph, 0.0, 0.3, 11.0, dir_range=(5, B), with_loss=False)) <= 1e-12


@pytest.mark.parametrize("shape", [(16, 16, 16), (32, 32, 32), (16, 8, 6)])
def test_g_equal_f_is_the_emulated_operator(oracle, shape):
    _, f = _fields(shape, seed=1)
    gl = oracle.gauss_legendre(2, 0.0, R)
    sph = BR.random_rule(6)
    d_Q = E.collide(f, gl, sph, 0.0, 0.3, 11.0, 64)[0]
    for same in (False, True):
        Q = emu_bilinear(f.copy(), f, gl, sph, 0.0, 0.3, 11.0, same=same)
        assert _rel(Q, d_Q) <= 1e-14, (shape, same)


def test_exact_reduction_handles_are_refused():
    g, f = _fields((16, 16, 16))
    gl = (np.array([3.0]), np.array([1.0]))
    with pytest.raises(RuntimeError, match="rc=2"):
        emu_bilinear(g, f, gl, BR.random_rule(4), 0.0, 0.3, 11.0, flags=2)


# ---- the fused-cube case table of the GPU suite (tests/bilinear_cases.py) -----------------------------------------

def _pipeline_text():
    return open(os.path.join(PKG, "csrc", "bfsm_pipeline.hpp")).read()


def test_every_fused_cube_has_a_bilinear_gpu_case():
    """Every cube size of fused_grid() in both precisions has exactly one case, and nothing else does: a new fused size
    cannot slip in without a GPU case."""
    sizes = BC.fused_sizes_of_pipeline(_pipeline_text())
    assert 16 in sizes and 128 in sizes, sizes
    required = {(n, p) for n in sizes for p in (64, 32)}
    declared = [(c.n, c.prec) for c in BC.CUBES]
    assert len(declared) == len(set(declared)), "a (N, precision) pair declared twice"
    assert not required - set(declared), f"fused cubes without a bilinear GPU case: {sorted(required - set(declared))}"
    assert not set(declared) - required, f"cases that are not fused cubes: {sorted(set(declared) - required)}"
    for c in BC.CUBES:
        assert c.geometry and c.n_gl >= 1 and c.n_sph >= 3, c


def test_launch_variants_take_their_declared_plan():
    """Each variant's chunks and slabs under the library's own make_plan, and so the reduce route: the separate Reduce
    launch above fuse_reduce()'s slab limit, the reduce fused into the tail at or below it.  The chunked variants cross a
    radial-node boundary inside a chunk; every size has one variant of each route."""
    limit = int(re.search(r"bool fuse_reduce\(\) const \{ return slab_count <= (\d+); \}", _pipeline_text()).group(1))
    routes = {}
    for v in BC.VARIANTS:
        c = BC.cube(v.n, v.prec)
        chunks, segs = E.plan(v.n, c.n_gl, c.n_sph, v.prec, max_chunk=v.max_chunk)
        assert (len(chunks), len(segs)) == (v.chunks, v.slabs), v
        assert v.reduce == (1 if v.slabs > limit else 0), v
        if v.max_chunk:
            assert v.chunks > 1 and any(d0 // c.n_sph != (d0 + n - 1) // c.n_sph for _, d0, n, _, _ in chunks), v
        routes.setdefault((v.n, v.prec), set()).add((v.chunks > 1, v.reduce))
    assert set(routes) == set(BC.VARIANT_SIZES)
    for key, r in routes.items():
        assert r == {(True, 1), (False, 0)}, key
    for n, prec in BC.VARIANT_SIZES:
        c = BC.cube(n, prec)
        sh = BC.shards(c.n_gl * c.n_sph)
        assert len(sh) == 3 and sh[0][0] == 0 and sh[-1][1] == c.n_gl * c.n_sph
        assert all(a[1] == b[0] for a, b in zip(sh, sh[1:])) and len({b - a for a, b in sh}) == 3, sh


# ---- the C-ABI without a GPU ------------------------------------------------------------------------------------

def test_null_handle_is_invalid_without_gpu():
    so = os.path.join(PKG, "libbfsm_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", PKG, "-s", "libbfsm_hip.so"])
    from bfsm import capi
    L = capi.load_library()
    q = (ctypes.c_double * 8)()
    assert L.bfsm_collide_bilinear(None, q, q, q) == 1   # BFSM_ERR_INVALID
    assert L.bfsm_collide_bilinear_async(None, q, q, q, None) == 1   # BFSM_ERR_INVALID
    assert L.bfsm_collide_bilinear_partial_async(None, q, q, q, 1, None) == 1   # BFSM_ERR_INVALID
