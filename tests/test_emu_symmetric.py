"""CPU tests of the symmetric form Qs(g,f) = Q(g,f) + Q(f,g) (include/bfsm.h, bfsm_collide_symmetric*).

The launch sequence of bfsm_collide_symmetric_partial_async (csrc/bfsm_calls.hpp, collide_symmetric) and its kernel bodies run
under the host lock-step emulator (tests/emu/bfsm_emu_symmetric.cpp, built into its own library with the flags of
tests/emu/Makefile) and are compared with tests/symmetric_ref.py, two reference evaluations on the full rule: N = 16 and 24 in
the three modes and N = 32 exact + Hermitian, each with an antipodal rule (merged by the exact modes) and one without that
symmetry; Qs(f,f) against twice the oracle, the symmetry in (g,f), shards on a merged plan, a size-generic box.  The case table
of the GPU suite (tests/symmetric_cases.py) is checked against fused_grid() and make_plan, and every antipodal case shows that
it tells the operator from a single merged pass.  Bounds: tests/test_gpu_bilinear.py's, 1e-12 in fp64 and 5e-6 in fp32, relative
to max|reference|.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bilinear_cases as BC
import bilinear_ref as BR
import emu_lib as E
import symmetric_cases as SC
import symmetric_ref as SR
from test_emu_bilinear import _emu_flags

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd")
TOL64, TOL32 = 1e-12, 5e-6                  # tests/test_gpu_bilinear.py
TEETH = 1000.0                              # the wrong operator lies at least this many bounds from the reference
GAMMA, B_GAMMA, L_BOX, R_MAX = 0.5, 0.3, 11.0, 10.0

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "bfsm_emu_symmetric.cpp")
        so = os.path.join(HERE, "emu", "libbfsm_emu_symmetric.so")
        deps = [src, os.path.join(HERE, "emu", "bfsm_emu.cpp"), os.path.join(ROOT, "include", "bfsm.h")] + \
               [os.path.join(PKG, "csrc", n) for n in ("bfsm_core.hpp", "bfsm_pipeline.hpp", "bfsm_generic.hpp", "bfsm_calls.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            tmp = so[:-3] + ".%d.tmp.so" % os.getpid()
            subprocess.check_call([os.environ.get("CXX", "g++")] + _emu_flags() + ["-o", tmp, src])
            os.replace(tmp, so)
        from bfsm import capi
        L = ctypes.CDLL(so)
        dp = ctypes.POINTER(ctypes.c_double)
        L.bfsm_emu_collide_symmetric.argtypes = [ctypes.POINTER(capi.Desc), dp, dp, dp, ctypes.c_int]
        L.bfsm_emu_collide_symmetric.restype = ctypes.c_int
        L.bfsm_emu_symmetric_plan.argtypes = [ctypes.POINTER(capi.Desc), ctypes.POINTER(ctypes.c_int)]
        L.bfsm_emu_symmetric_plan.restype = ctypes.c_int
        _LIB = L
    return _LIB


def emu_symmetric(g, f, gl, sph, precision=64, flags=0, dir_range=(0, 0), with_loss=True, same=False, max_chunk=0):
    """same=True passes f's buffer as g (the g == f pointer case of the C-ABI)."""
    nv = f.shape[0] if f.shape[0] == f.shape[1] == f.shape[2] else f.shape
    d, keep = E.make_desc(nv, gl, sph, GAMMA, B_GAMMA, L_BOX, precision, dir_range, max_chunk, flags)
    f = np.ascontiguousarray(f, dtype=np.float64)
    g = f if same else np.ascontiguousarray(g, dtype=np.float64)
    Q = np.empty_like(f)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib().bfsm_emu_collide_symmetric(ctypes.byref(d), g.ctypes.data_as(dp), f.ctypes.data_as(dp), Q.ctypes.data_as(dp),
                                          1 if with_loss else 0)
    if rc:
        raise RuntimeError(f"bfsm_emu_collide_symmetric rc={rc}")
    return Q


def plan_info(n, prec, flags, gl, sph, dir_range=(0, 0), max_chunk=0, max_batch=0):
    """(antipodal, sph_eff, weight_mult, hermitian, chunks, slabs) under the library's make_plan."""
    d, keep = E.make_desc(n, gl, sph, GAMMA, B_GAMMA, L_BOX, prec, dir_range, max_chunk, flags, max_batch)
    info = (ctypes.c_int * 6)()
    rc = lib().bfsm_emu_symmetric_plan(ctypes.byref(d), info)
    assert rc == 0, rc
    return tuple(info)


def fields(shape, seed):
    """g, f: sign-indefinite, without any symmetry, mutually different (the draw of test_gpu_bilinear_cubes._fields, shifted)."""
    rng = np.random.default_rng(seed)
    return rng.random(shape) - 0.45, rng.random(shape) - 0.45


def gauss_legendre(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * R_MAX * (x + 1.0), 0.5 * R_MAX * w


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _tol(prec):
    return TOL64 if prec == 64 else TOL32


def _ref(g, f, gl, sph, **kw):
    return SR.collide_symmetric(g, f, gl, sph, GAMMA, B_GAMMA, L_BOX, **kw)


# ---- the emulated kernels against the reference -----------------------------------------------------------------------

_SMALL = [(n, prec, mode) for n in (16, 24) for prec in (64, 32) for mode in ("faithful", "exact", "hermitian")] + \
         [(32, 64, "hermitian"), (32, 32, "hermitian")]


@pytest.mark.parametrize("rule", ["antipodal", "odd"])
@pytest.mark.parametrize("n,prec,mode", _SMALL)
def test_small_cubes_match_reference(n, prec, mode, rule):
    """Two radial nodes; the antipodal rule has 2 x 3 points (merged to 3 on the exact modes), the other 5 (never merged)."""
    g, f = fields((n, n, n), seed=n)
    gl = gauss_legendre(2)
    sph = SR.antipodal_rule(3, seed=n) if rule == "antipodal" else BR.random_rule(5, seed=n)
    ref = _ref(g, f, gl, sph)
    tol = _tol(prec)
    if rule == "antipodal":       # on the reference alone, before any device result: the case can see a missing exchanged product
        away = _rel(SR.wrong_merged(g, f, gl, sph, GAMMA, B_GAMMA, L_BOX), ref)
        assert away >= TEETH * tol, away
    flags = SC.MODES[mode]
    info = plan_info(n, prec, flags, gl, sph)
    assert info[0] == (1 if rule == "antipodal" and mode != "faithful" else 0)
    assert info[3] == (1 if mode == "hermitian" else 0)
    Q = emu_symmetric(g, f, gl, sph, prec, flags)
    err = _rel(Q, ref)
    print(f"N={n} fp{prec} {mode} {rule}: max rel err {err:.2e} (bound {tol:.0e})")
    assert err <= tol


@pytest.mark.parametrize("mode,max_chunk", [("hermitian", 2), ("exact", 2), ("faithful", 2), ("hermitian", 0)])
def test_chunks_across_radial_nodes_and_the_separate_reduce(mode, max_chunk):
    """N = 24, 3 radial nodes x 3 effective directions in chunks of 2: chunks cross the nodes, 2 x slabs > 8; and in one chunk."""
    n = 24
    g, f = fields((n, n, n), seed=5)
    gl = gauss_legendre(3)
    sph = SR.antipodal_rule(3, seed=2)
    Q = emu_symmetric(g, f, gl, sph, 64, SC.MODES[mode], max_chunk=max_chunk)
    assert _rel(Q, _ref(g, f, gl, sph)) <= TOL64


@pytest.mark.parametrize("n,mode", [(16, "hermitian"), (24, "exact"), (16, "faithful")])
def test_twice_the_operator_and_symmetry(oracle, n, mode):
    """Qs(f,f) = 2 Q(f,f) (oracle), through one pointer and through two; Qs(g,f) = Qs(f,g)."""
    g, f = fields((n, n, n), seed=n + 1)
    gl = gauss_legendre(2)
    sph = SR.antipodal_rule(3, seed=n)
    flags = SC.MODES[mode]
    two_q = 2 * oracle.collide(f, gl, sph, GAMMA, B_GAMMA, L_BOX)
    assert _rel(emu_symmetric(f.copy(), f, gl, sph, 64, flags), two_q) <= TOL64
    assert _rel(emu_symmetric(f, f, gl, sph, 64, flags, same=True), two_q) <= TOL64
    a, b = emu_symmetric(g, f, gl, sph, 64, flags), emu_symmetric(f, g, gl, sph, 64, flags)
    assert float(np.abs(a - b).max() / np.abs(a).max()) <= TOL64


@pytest.mark.parametrize("mode", ["hermitian", "exact"])
def test_three_uneven_shards_sum_to_the_whole_on_a_merged_plan(mode):
    n = 24
    g, f = fields((n, n, n), seed=8)
    gl = gauss_legendre(2)
    sph = SR.antipodal_rule(5, seed=3)                  # 20 full directions, 10 effective
    flags = SC.MODES[mode]
    total = np.zeros_like(f)
    for rank, rng in enumerate(BC.shards(20)):
        assert plan_info(n, 64, flags, gl, sph, dir_range=rng)[0] == 1
        total += emu_symmetric(g, f, gl, sph, 64, flags, dir_range=rng, with_loss=(rank == 0))
    assert _rel(total, _ref(g, f, gl, sph)) <= TOL64


@pytest.mark.parametrize("shape,prec", [((12, 8, 20), 64), ((12, 6, 10), 32), ((8, 14, 6), 64)])
def test_size_generic_boxes_match_reference(shape, prec):
    """The fused sequence in both precisions and the x-line sequence behind per-axis passes; a shard without the loss terms."""
    g, f = fields(shape, seed=sum(shape))
    gl = gauss_legendre(2)
    sph = BR.random_rule(5, seed=sum(shape))
    assert _rel(emu_symmetric(g, f, gl, sph, prec), _ref(g, f, gl, sph)) <= _tol(prec)
    part = emu_symmetric(g, f, gl, sph, prec, dir_range=(3, 8), with_loss=False)
    assert _rel(part, _ref(g, f, gl, sph, dir_range=(3, 8), with_loss=False)) <= _tol(prec)


# ---- the case table of the GPU suite (tests/symmetric_cases.py) ---------------------------------------------------------

def test_every_fused_cube_has_a_hermitian_case():
    sizes = BC.fused_sizes_of_pipeline(open(os.path.join(PKG, "csrc", "bfsm_pipeline.hpp")).read())
    required = {(n, p) for n in sizes for p in (64, 32)}
    declared = [(c.shape, c.prec) for c in SC.CASES if c.mode == "hermitian"]
    assert len(declared) == len(set(declared)) and set(declared) == required
    keys = [(c.shape, c.prec, c.mode) for c in SC.CASES]
    assert len(keys) == len(set(keys))
    for want in [(16, 64, "exact"), (32, 64, "exact"), (64, 64, "exact"), (128, 32, "exact"), (16, 64, "faithful"),
                 (32, 64, "faithful"), (64, 64, "faithful"), ((12, 8, 20), 64, "faithful"), ((20, 20, 20), 64, "faithful")]:
        assert want in keys, want


def _groups(n, mode):
    """Pipeline::gain_spectra, groups_a (max_batch <= 1)."""
    target = 512 if n >= 64 else (2048 if n == 32 else 1024)
    planes = n // 2 + 1 if mode == "hermitian" else n
    return max(target // planes, 1) * (2 if n == 64 else 1)


@pytest.mark.parametrize("c", [c for c in SC.CASES if isinstance(c.shape, int)], ids=SC.cid)
def test_cases_take_their_declared_plan(c):
    gl = gauss_legendre(c.n_gl)
    sph = SR.antipodal_rule(c.n_sph // 2, seed=c.shape)
    anti, sph_eff, mult, herm, chunks, slabs = plan_info(c.shape, c.prec, SC.MODES[c.mode], gl, sph)
    merged = c.mode != "faithful"
    assert (anti, mult, herm) == (int(merged), 2 if merged else 1, int(c.mode == "hermitian")), c
    assert (sph_eff, chunks, slabs) == (c.sph_eff, c.chunks, c.slabs), (c, sph_eff, chunks, slabs)
    assert c.groups == _groups(c.shape, c.mode) and c.loop == (c.n_gl * c.sph_eff > c.groups), c
    assert 2 <= c.n_gl <= 5 and 5 <= c.n_sph <= 14, c


def test_variants_take_their_declared_plan():
    routes = {}
    for v in SC.VARIANTS:
        c = SC.case(v.n, v.prec, "hermitian")
        gl = gauss_legendre(c.n_gl)
        sph = SR.antipodal_rule(c.n_sph // 2, seed=c.shape)
        info = plan_info(v.n, v.prec, SC.MODES["hermitian"], gl, sph, v.shard or (0, 0), v.max_chunk, v.max_batch)
        assert info[0] == 1 and (info[4], info[5]) == (v.chunks, v.slabs), (v, info)
        assert v.reduce == (1 if 2 * v.slabs > SC.FUSE_LIMIT else 0), v
        if v.kind == "chunks":
            chunks, _ = E.plan(v.n, c.n_gl, c.n_sph, v.prec, max_chunk=v.max_chunk, flags=SC.MODES["hermitian"], sph=sph)
            assert any(d0 // c.sph_eff != (d0 + n - 1) // c.sph_eff for _, d0, n, _, _ in chunks), v
        routes.setdefault((v.n, v.prec), set()).add((v.kind, v.reduce))
    assert set(routes) == set(SC.VARIANT_SIZES)
    for r in routes.values():
        assert {("chunks", 1), ("single", 0)} <= r and "batch" in {k for k, _ in r}


# the reference alone, on the inputs the GPU suite uses: every antipodal case tells Qs from one merged pass without the
# exchanged product.  Sizes up to 48 here (the larger ones assert the same on the GPU machine before they run: minutes of numpy)
@pytest.mark.parametrize("c", [c for c in SC.CASES if isinstance(c.shape, int) and c.shape <= 48 and c.prec == 64], ids=SC.cid)
def test_antipodal_cases_have_teeth(c):
    inp = gpu_inputs(c)
    assert inp["away"] >= TEETH * TOL32, inp["away"]


_INPUTS = {}


def gpu_inputs(c):
    """g, f, the quadratures, the reference Qs(g,f) and the distance of the wrong (single merged pass) operator of a case;
    computed once per (shape, n_gl, n_sph), shared by both precisions and every test, never modified."""
    key = (c.shape, c.n_gl, c.n_sph)
    if key not in _INPUTS:
        shape = (c.shape,) * 3 if isinstance(c.shape, int) else c.shape
        seed = c.shape if isinstance(c.shape, int) else sum(c.shape)
        g, f = fields(shape, seed)
        gl = gauss_legendre(c.n_gl)
        sph = SR.antipodal_rule(c.n_sph // 2, seed=seed)
        ref = _ref(g, f, gl, sph)
        away = _rel(SR.wrong_merged(g, f, gl, sph, GAMMA, B_GAMMA, L_BOX), ref)
        for a in (g, f, ref):
            a.setflags(write=False)
        _INPUTS[key] = dict(g=g, f=f, gl=gl, sph=sph, ref=ref, away=away)
    return _INPUTS[key]


# ---- the C-ABI without a GPU --------------------------------------------------------------------------------------------

def test_null_handle_is_invalid_without_gpu():
    so = os.path.join(PKG, "libbfsm_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", PKG, "-s", "libbfsm_hip.so"])
    from bfsm import capi
    L = capi.load_library()
    q = (ctypes.c_double * 8)()
    assert L.bfsm_collide_symmetric(None, q, q, q) == 1
    assert L.bfsm_collide_symmetric_async(None, q, q, q, None) == 1
    assert L.bfsm_collide_symmetric_partial_async(None, q, q, q, 1, None) == 1
