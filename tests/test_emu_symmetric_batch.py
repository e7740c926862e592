"""CPU tests of the batched two-operand forms (include/bfsm.h, bfsm_collide_symmetric_batch*, bfsm_collide_bilinear_batch_partial_async).

The library's own launch sequence (csrc/bfsm_calls.hpp, collide_pairs) and its kernel bodies run under the host lock-step emulator
(tests/emu/bfsm_emu_symmetric_batch.cpp, built into its own library with the flags of tests/emu/Makefile) for the N = 16 / 24 / 32
cases and the box of tests/symmetric_batch_cases.py, against tests/symmetric_ref.py / tests/bilinear_ref.py per member on the full
rule.  Bounds: tests/test_gpu_bilinear.py's, 1e-12 in fp64 and 5e-6 in fp32, relative to max|reference|.  Member i is bitwise the
single emulated call; a shared operand is bitwise the replicated one; the input transforms run n_batch + 1 times with a shared
operand and 2 n_batch without.  Before any device result the reference alone shows that a case has teeth: the members' references
differ by at least 1000 bounds, and so does the reference with the wrong operand shared.  The stand-alone sanitizer program
tests/emu/symmetric_batch_sanitize_main.cpp is built and run here as well.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bilinear_ref as BR
import emu_lib as E
import symmetric_batch_cases as SB
import symmetric_ref as SR
from test_emu_bilinear import _emu_flags
from test_emu_symmetric import B_GAMMA, GAMMA, L_BOX, TEETH, _rel, _tol, gauss_legendre, plan_info

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd")
K_TILE_FWD_REAL, K_LINE_FWD, K_REDUCE, K_TAIL_INV, K_TAIL_LINE = 0, 1, 8, 9, 10          # enum class K, csrc/bfsm_pipeline.hpp

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emu", "bfsm_emu_symmetric_batch.cpp")
        so = os.path.join(HERE, "emu", "libbfsm_emu_symmetric_batch.so")
        deps = [src, os.path.join(HERE, "emu", "bfsm_emu.cpp"), os.path.join(ROOT, "include", "bfsm.h")] + \
               [os.path.join(PKG, "csrc", n) for n in ("bfsm_core.hpp", "bfsm_pipeline.hpp", "bfsm_generic.hpp", "bfsm_calls.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            tmp = so[:-3] + ".%d.tmp.so" % os.getpid()
            subprocess.check_call([os.environ.get("CXX", "g++")] + _emu_flags() + ["-o", tmp, src])
            os.replace(tmp, so)
        from bfsm import capi
        L = ctypes.CDLL(so)
        dp, ip, ci = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int
        L.bfsm_emu_collide_pairs.argtypes = [ctypes.POINTER(capi.Desc), dp, dp, dp, ci, ci, ci, ci, ip]
        L.bfsm_emu_collide_pairs.restype = ci
        L.bfsm_emu_collide_pair_single.argtypes = [ctypes.POINTER(capi.Desc), dp, dp, dp, ci, ci, ip]
        L.bfsm_emu_collide_pair_single.restype = ci
        _LIB = L
    return _LIB


def _desc(c):
    inp = batch_inputs(c)
    return E.make_desc(c.shape, inp["gl"], inp["sph"], GAMMA, B_GAMMA, L_BOX, c.prec, c.shard or (0, 0), c.max_chunk,
                       SB.MODES[c.mode], c.max_batch)


def emu_pairs(c, g, f, n_batch, share, symmetric=True, with_loss=True):
    """(Q [n_batch][shape], launches by kernel kind) of the emulated batched call."""
    from bfsm import capi
    d, keep = _desc(c)
    g, f = np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(f, dtype=np.float64)
    Q = np.full((n_batch,) + g.shape[-3:], np.nan)
    dp = ctypes.POINTER(ctypes.c_double)
    launches = (ctypes.c_int * 64)()
    rc = lib().bfsm_emu_collide_pairs(ctypes.byref(d), g.ctypes.data_as(dp), f.ctypes.data_as(dp), Q.ctypes.data_as(dp), n_batch,
                                      capi.SHARE[share], 1 if with_loss else 0, 1 if symmetric else 0, launches)
    if rc:
        raise RuntimeError(f"bfsm_emu_collide_pairs rc={rc}")
    return Q, tuple(launches)


def emu_single(c, g, f, symmetric=True, with_loss=True):
    d, keep = _desc(c)
    g, f = np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(f, dtype=np.float64)
    Q = np.full(g.shape, np.nan)
    dp = ctypes.POINTER(ctypes.c_double)
    launches = (ctypes.c_int * 64)()
    rc = lib().bfsm_emu_collide_pair_single(ctypes.byref(d), g.ctypes.data_as(dp), f.ctypes.data_as(dp), Q.ctypes.data_as(dp),
                                            1 if with_loss else 0, 1 if symmetric else 0, launches)
    if rc:
        raise RuntimeError(f"bfsm_emu_collide_pair_single rc={rc}")
    return Q, tuple(launches)


# ---- inputs and references, computed once and shared by the CPU and the GPU suite, never modified ------------------------------

_INPUTS, _REFS = {}, {}


def batch_inputs(c):
    """SB.MAX_BATCH distributions g_i and f_i (sign-indefinite, without symmetry, mutually different) and the quadratures."""
    key = (c.shape, c.n_gl, c.n_sph)
    if key not in _INPUTS:
        shape = (c.shape,) * 3 if isinstance(c.shape, int) else c.shape
        seed = c.shape if isinstance(c.shape, int) else sum(c.shape)
        rng = np.random.default_rng(1000 + seed)
        g, f = rng.random((SB.MAX_BATCH,) + shape) - 0.45, rng.random((SB.MAX_BATCH,) + shape) - 0.45
        for a in (g, f):
            a.setflags(write=False)
        _INPUTS[key] = dict(g=g, f=f, gl=gauss_legendre(c.n_gl), sph=SR.antipodal_rule(c.n_sph // 2, seed=seed))
    return _INPUTS[key]


def operands(c, share=None, n_batch=None):
    """(g, f) as the call takes them: [n_batch][shape], or one array for the shared operand (member 0's)."""
    inp = batch_inputs(c)
    share = c.share if share is None else (None if share == "none" else share)
    nb = n_batch or c.n_batch
    return (inp["g"][0] if share == "g" else inp["g"][:nb]), (inp["f"][0] if share == "f" else inp["f"][:nb])


def member_ref(c, i, share, symmetric=True, shard=None):
    """Reference of member i under `share`: Qs(g_j, f_k) / Q(g_j, f_k) with j = 0 if g is shared else i, k likewise."""
    j, k = (0 if share == "g" else i), (0 if share == "f" else i)
    key = (c.shape, c.n_gl, c.n_sph, j, k, symmetric, shard)
    if key not in _REFS:
        inp = batch_inputs(c)
        sph, rng = inp["sph"], None
        if shard is not None:
            # a shard of a merged plan is a range of EFFECTIVE directions (make_plan: b * sph_eff / n_sph), each an antipodal pair:
            # the reference on the half rule with doubled weights over that range (tests/test_gpu_symmetric.py)
            sph, rng = SR.half_rule_doubled(sph), tuple(b * (c.n_sph // 2) // c.n_sph for b in shard)
        fn = SR.collide_symmetric if symmetric else BR.collide_bilinear
        ref = fn(inp["g"][j], inp["f"][k], inp["gl"], sph, GAMMA, B_GAMMA, L_BOX, rng) if rng else \
            fn(inp["g"][j], inp["f"][k], inp["gl"], sph, GAMMA, B_GAMMA, L_BOX)
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def case_ref(c, i):
    assert c.shard is None or c.mode != "faithful"
    return member_ref(c, i, c.share, True, c.shard)


def assert_teeth(c):
    """On the reference alone: the members differ from each other, and sharing the wrong operand (or none, or both) is seen."""
    if c.n_batch < 2:
        return
    tol = _tol(c.prec)
    refs = [case_ref(c, i) for i in range(c.n_batch)]
    for i in range(1, c.n_batch):
        away = _rel(refs[i], refs[0])
        assert away >= TEETH * tol, (SB.cid(c), i, away)
    for wrong in (s for s in SB.SHARES if s != c.share):
        away = _rel(member_ref(c, 1, wrong, True, c.shard), refs[1])
        print(f"{SB.cid(c)}: member 1 with share={wrong} lies at {away:.2e} from the reference")
        assert away >= TEETH * tol, (SB.cid(c), wrong, away)


# ---- the emulated sequence against the reference --------------------------------------------------------------------------------

@pytest.mark.parametrize("c", SB.EMU_CASES, ids=SB.cid)
def test_case_matches_reference_and_the_single_call(c):
    assert_teeth(c)
    g, f = operands(c)
    tol = _tol(c.prec)
    Q, launches = emu_pairs(c, g, f, c.n_batch, c.share)
    for i in range(c.n_batch):
        err = _rel(Q[i], case_ref(c, i))
        print(f"{SB.cid(c)} member {i}: max rel err {err:.2e} (bound {tol:.0e})")
        assert err <= tol
    # member i is bitwise the single call on a handle of the same descriptor, whatever the others hold
    inp = batch_inputs(c)
    for i in range(c.n_batch):
        one, _ = emu_single(c, inp["g"][0 if c.share == "g" else i], inp["f"][0 if c.share == "f" else i])
        assert np.array_equal(one, Q[i]), (SB.cid(c), i)
    if isinstance(c.shape, int):
        # the two launches of an input transform carry its members in grid.y: n_batch + 1 transforms with a shared operand
        transforms = c.n_batch + 1 if c.share else 2 * c.n_batch
        assert launches[K_TILE_FWD_REAL] == launches[K_LINE_FWD] == 2
        assert launches[32 + K_TILE_FWD_REAL] == launches[32 + K_LINE_FWD] == transforms, launches
        assert launches[K_REDUCE] == c.reduce and launches[K_TAIL_INV] == 1 and launches[K_TAIL_LINE] == 1


_REPL = [c for c in SB.EMU_CASES if c.share and c.n_batch >= 2 and c.prec == 64]


@pytest.mark.parametrize("c", _REPL, ids=SB.cid)
def test_shared_operand_equals_the_replicated_one(c):
    g, f = operands(c)
    Q, _ = emu_pairs(c, g, f, c.n_batch, c.share)
    gr = np.broadcast_to(g, (c.n_batch,) + g.shape[-3:]) if c.share == "g" else g
    fr = np.broadcast_to(f, (c.n_batch,) + f.shape[-3:]) if c.share == "f" else f
    R, _ = emu_pairs(c, gr, fr, c.n_batch, None)
    assert np.array_equal(Q, R)


@pytest.mark.parametrize("share", ["none", "g", "f"])
def test_bilinear_batch_on_a_faithful_handle(share):
    c = [k for k in SB.CASES if (k.shape, k.prec, k.mode, k.n_batch) == (16, 64, "faithful", 3)][0]
    sh = None if share == "none" else share
    g, f = operands(c, share)
    Q, _ = emu_pairs(c, g, f, 3, sh, symmetric=False)
    inp = batch_inputs(c)
    for i in range(3):
        assert _rel(Q[i], member_ref(c, i, sh, symmetric=False)) <= _tol(64)
        one, _ = emu_single(c, inp["g"][0 if sh == "g" else i], inp["f"][0 if sh == "f" else i], symmetric=False)
        assert np.array_equal(one, Q[i])


def test_input_transforms_cover_n_batch_plus_one_members_with_a_shared_operand():
    """Launch record: the input-transform kernels run for n_batch + 1 members with a shared operand and 2 n_batch without; one
    sequence for the whole batch; a batch of one takes the launches of the single call."""
    c = [k for k in SB.CASES if (k.shape, k.prec, k.mode, k.n_batch) == (16, 64, "hermitian", 3)][0]
    inp = batch_inputs(c)
    _, single = emu_single(c, inp["g"][0], inp["f"][0])
    _, one = emu_pairs(c, inp["g"][:1], inp["f"][:1], 1, None)
    assert one == single
    for share in SB.SHARES:
        g, f = operands(c, share or "none", 3)
        _, rec = emu_pairs(c, g, f, 3, share)
        assert rec[:32] == single[:32], (share, rec, single)            # one sequence for the whole batch
        assert rec[32 + K_TILE_FWD_REAL] == rec[32 + K_LINE_FWD] == (3 + 1 if share else 2 * 3), (share, rec)


def test_argument_errors_of_the_sequence():
    c = [k for k in SB.CASES if (k.shape, k.prec, k.mode, k.n_batch) == (16, 64, "exact", 3)][0]
    g, f = operands(c, "none", 3)
    with pytest.raises(RuntimeError, match="rc=1"):
        emu_pairs(c, g, f, SB.MAX_BATCH + 1, None)
    with pytest.raises(RuntimeError, match="rc=2"):
        emu_pairs(c, g, f, 3, None, symmetric=False)          # the bilinear form on an exact-reduction handle


# ---- the case table against make_plan --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in SB.CASES if isinstance(c.shape, int)], ids=SB.cid)
def test_cases_take_their_declared_plan(c):
    inp = batch_inputs(c) if c.shape <= 32 else dict(gl=gauss_legendre(c.n_gl), sph=SR.antipodal_rule(c.n_sph // 2, seed=c.shape))
    anti, eff, mult, herm, chunks, slabs = plan_info(c.shape, c.prec, SB.MODES[c.mode], inp["gl"], inp["sph"], c.shard or (0, 0),
                                                     c.max_chunk, c.max_batch)
    assert (anti, herm) == (int(c.mode != "faithful"), int(c.mode == "hermitian")), c
    assert (eff, chunks, slabs) == (SB.sph_eff(c), c.chunks, c.slabs), (c, eff, chunks, slabs)
    assert c.reduce == (1 if 2 * c.slabs > SB.FUSE_LIMIT else 0), c
    assert 1 <= c.n_batch <= c.max_batch


def test_table_reaches_every_kernel_form():
    keys = {(c.shape, c.prec, c.mode) for c in SB.CASES}
    for n in (16, 24):
        for prec in (64, 32):
            for mode in SB.MODES:
                mine = [c for c in SB.CASES if (c.shape, c.prec, c.mode) == (n, prec, mode) and not c.max_chunk and not c.shard]
                assert sorted(c.n_batch for c in mine) == [1, 2, 3] and {c.share for c in mine} == set(SB.SHARES)
    assert {(32, 64, "hermitian"), (64, 64, "hermitian"), (64, 64, "faithful"), (128, 32, "hermitian"), ((12, 8, 20), 64, "faithful")} <= keys
    n64 = [c for c in SB.CASES if (c.shape, c.mode) == (64, "hermitian")][0]
    assert n64.n_gl * SB.sph_eff(n64) > SB.groups(64, "hermitian", n64.max_batch)          # KA's workgroups loop over two directions
    n128 = [c for c in SB.CASES if c.shape == 128][0]
    assert (n128.share, n128.n_gl, n128.n_sph // 2) == ("f", 1, 4)
    assert any(c.max_chunk == 2 and c.reduce == 1 and c.n_batch == 2 for c in SB.CASES)
    assert any(c.shard and c.reduce == 0 and c.n_batch == 2 for c in SB.CASES)


# ---- the stand-alone sanitizer program ---------------------------------------------------------------------------------------------

def test_sanitizer_program_runs_clean(tmp_path):
    """tests/emu/symmetric_batch_sanitize_main.cpp under -fsanitize=address,undefined (its own main: nothing is preloaded)."""
    cxx = os.environ.get("CXX", "g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined"]
    if subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no AddressSanitizer / UBSan runtime")
    exe = str(tmp_path / "symmetric_batch_sanitize")
    subprocess.check_call([cxx, "-O1", "-g1", "-std=c++17"] + san + ["-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                           "-DBFSM_FUSED_N_MAX=24", "-o", exe, os.path.join(HERE, "emu", "symmetric_batch_sanitize_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1800, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "symmetric batch sanitizer run: clean" in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr


# ---- the C-ABI without a GPU -------------------------------------------------------------------------------------------------------

def test_null_handle_is_invalid_without_gpu():
    so = os.path.join(PKG, "libbfsm_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", PKG, "-s", "libbfsm_hip.so"])
    from bfsm import capi
    L = capi.load_library()
    q = (ctypes.c_double * 8)()
    assert L.bfsm_collide_symmetric_batch(None, q, q, q, 1, 0) == 1
    assert L.bfsm_collide_symmetric_batch_partial_async(None, q, q, q, 1, 0, 1, None) == 1
    assert L.bfsm_collide_bilinear_batch_partial_async(None, q, q, q, 1, 0, 1, None) == 1
