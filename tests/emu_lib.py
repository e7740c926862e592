"""ctypes access to tests/emu/libbfsm_emu.so -- the host lock-step emulation of the HIP kernel bodies (test harness)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_LIB512 = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu"), "-s"])
        # BFSM_EMU_LIB: an alternative build of the same emulator (the AddressSanitizer build of tests/emu/Makefile)
        _LIB = _typed(ctypes.CDLL(os.environ.get("BFSM_EMU_LIB") or os.path.join(_HERE, "emu", "libbfsm_emu.so")))
    return _LIB


def lib_gpu_groups():
    """The emulator built with the library's own plane-accumulate grouping (512 workgroups per launch, as on the GPU;
    lib() asks for 24 so that small cases give every group several directions)."""
    global _LIB512
    if _LIB512 is None:
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "emu"), "-s"])
        _LIB512 = _typed(ctypes.CDLL(os.path.join(_HERE, "emu", "libbfsm_emu_wgs512.so")))
    return _LIB512


def _typed(L):
    from bfsm import capi
    dp = ctypes.POINTER(ctypes.c_double)
    L.bfsm_emu_collide.argtypes = [ctypes.POINTER(capi.Desc), dp, dp, dp]
    L.bfsm_emu_collide.restype = ctypes.c_int
    L.bfsm_emu_fft3d.argtypes = [ctypes.c_int, ctypes.c_int, dp, ctypes.c_int, ctypes.c_int]
    L.bfsm_emu_fft3d.restype = ctypes.c_int
    ip = ctypes.POINTER(ctypes.c_int)
    L.bfsm_emu_plan.argtypes = [ctypes.POINTER(capi.Desc), ip, ctypes.c_int, ip, ctypes.c_int, ip]
    L.bfsm_emu_plan.restype = ctypes.c_int
    L.bfsm_emu_gen_routes.argtypes = [ctypes.POINTER(capi.Desc), ctypes.c_int, ctypes.c_int, ip, ctypes.c_int, ip, ip,
                                      ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    L.bfsm_emu_gen_routes.restype = ctypes.c_int
    L.bfsm_emu_collide_batch.argtypes = [ctypes.POINTER(capi.Desc), dp, dp, dp, ctypes.c_int]
    L.bfsm_emu_collide_batch.restype = ctypes.c_int
    L.bfsm_emu_finish.argtypes = [ctypes.POINTER(capi.Desc), dp, dp, dp, ctypes.c_int]
    L.bfsm_emu_finish.restype = ctypes.c_int
    L.bfsm_emu_collide_partial.argtypes = [ctypes.POINTER(capi.Desc), dp, dp, ctypes.c_int]
    L.bfsm_emu_collide_partial.restype = ctypes.c_int
    return L


def make_desc(nv, gl, sph, gamma, b_gamma, L, precision=64, dir_range=(0, 0), max_chunk=0, flags=0, max_batch=0):
    """gl = (nodes, weights), sph = (x, y, z, w).  Returns (Desc, keepalive)."""
    from bfsm import capi
    dp = ctypes.POINTER(ctypes.c_double)
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (gl[0], gl[1], sph[3], sph[0], sph[1], sph[2])]
    nx, ny, nz = (nv, nv, nv) if np.isscalar(nv) else (int(v) for v in nv)     # nv: one extent or (nvx, nvy, nvz)
    d = capi.Desc(nx, ny, nz, len(keep[0]), len(keep[2]), *[a.ctypes.data_as(dp) for a in keep],
                  gamma, b_gamma, L, precision, 0, dir_range[0], dir_range[1], max_chunk, flags, max_batch)
    return d, keep


def collide(f, gl, sph, gamma, b_gamma, L, precision=64, dir_range=(0, 0), max_chunk=0, want_Q=True, flags=0, gpu_groups=False):
    """gpu_groups: run the build with the library's plane-accumulate grouping (lib_gpu_groups)."""
    nv = f.shape[0] if f.shape[0] == f.shape[1] == f.shape[2] else f.shape
    d, keep = make_desc(nv, gl, sph, gamma, b_gamma, L, precision, dir_range, max_chunk, flags)
    f = np.ascontiguousarray(f, dtype=np.float64)
    Q = np.empty_like(f)
    qh = np.empty(f.shape + (2,))
    dp = ctypes.POINTER(ctypes.c_double)
    rc = (lib_gpu_groups() if gpu_groups else lib()).bfsm_emu_collide(ctypes.byref(d), f.ctypes.data_as(dp), Q.ctypes.data_as(dp) if want_Q else None,
                                qh.ctypes.data_as(dp))
    if rc:
        raise RuntimeError(f"bfsm_emu_collide rc={rc}")
    qhat_t = qh[..., 0] + 1j * qh[..., 1]            # fused pipeline: [lx][lz][ly]; size-generic path: natural
    if np.isscalar(nv) and nv in (16, 24, 32, 40, 48, 64, 80, 96, 128):
        qhat_t = np.ascontiguousarray(qhat_t.transpose(0, 2, 1))   # -> [lx][ly][lz]
    return (Q if want_Q else None), qhat_t


def fft3d(a, sign, precision=64):
    """a: [batch][N][N][N] complex.  forward: natural in, natural out (un-transposed here); backward likewise."""
    a = np.ascontiguousarray(a, dtype=np.complex128)
    batch, n = a.shape[0], a.shape[1]
    if sign > 0:
        a = np.ascontiguousarray(a.transpose(0, 1, 3, 2))       # natural spectral -> [lx][lz][ly]
    buf = a.copy()
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib().bfsm_emu_fft3d(n, precision, buf.view(np.float64).ctypes.data_as(dp), batch, sign)
    if rc:
        raise RuntimeError(f"bfsm_emu_fft3d rc={rc}")
    if sign < 0:
        buf = np.ascontiguousarray(buf.transpose(0, 1, 3, 2))   # [lx][lz][ly] -> natural
    return buf


def plan(nv, n_gl, n_sph, precision=64, dir_range=(0, 0), max_chunk=0, flags=0, sph=None, max_batch=0):
    """Returns (chunks, segments): chunk rows (n_seg, dir0, n, per_group, seg0), segment rows (chunk, d0, n, r)."""
    gl = (np.ones(n_gl), np.ones(n_gl))
    if sph is None:
        sph = (np.ones(n_sph), np.zeros(n_sph), np.zeros(n_sph), np.ones(n_sph))
    d, keep = make_desc(nv, gl, sph, 0.0, 1.0, 1.0, precision, dir_range, max_chunk, flags, max_batch)
    crow = (ctypes.c_int * (5 * 4096))()
    srow = (ctypes.c_int * (5 * 65536))()
    nseg = ctypes.c_int()
    n = lib().bfsm_emu_plan(ctypes.byref(d), crow, 4096, srow, 65536, ctypes.byref(nseg))
    if n < 0:
        raise ValueError(f"plan rejected rc={-n}")
    return ([tuple(crow[5 * i:5 * i + 5]) for i in range(n)],
            [tuple(srow[5 * i:5 * i + 4]) for i in range(nseg.value)])


class EmuOperator:
    """Host-emulated stand-in for bfsm.HIPBoltzmannOperator with the sharded interface (gainPartial / qhat / finish),
    used by the world-size-2 gloo tests of the multi-GPU logic.  CPU torch tensors instead of device tensors."""

    def __init__(self, nv, gl, sph, gamma, b_gamma, L, dir_range=(0, 0), max_chunk=0):
        import torch
        self.nv, self.gl, self.sph = nv, gl, sph
        self.args = (gamma, b_gamma, L)
        self.dir_range, self.max_chunk = dir_range, max_chunk
        self.qhat = torch.zeros(2 * nv ** 3, dtype=torch.float64)     # the "handle-owned" partial Q_gain_hat

    def gainPartial(self, f, stream=0):
        import torch
        d, keep = make_desc(self.nv, self.gl, self.sph, *self.args, 64, self.dir_range, self.max_chunk)
        fh = np.ascontiguousarray(f.numpy(), dtype=np.float64)
        qh = np.empty(2 * self.nv ** 3)
        dp = ctypes.POINTER(ctypes.c_double)
        rc = lib().bfsm_emu_collide(ctypes.byref(d), fh.ctypes.data_as(dp), None, qh.ctypes.data_as(dp))
        if rc:
            raise RuntimeError(f"bfsm_emu_collide rc={rc}")
        self.qhat.copy_(torch.from_numpy(qh))

    def finishPartial(self, Q, f, with_loss, stream=0):
        self.finish(Q, f, stream, with_loss=with_loss)

    def finish(self, Q, f, stream=0, with_loss=True):
        import torch
        L = lib()
        dp = ctypes.POINTER(ctypes.c_double)
        d, keep = make_desc(self.nv, self.gl, self.sph, *self.args, 64, self.dir_range, self.max_chunk)
        fh = np.ascontiguousarray(f.numpy(), dtype=np.float64)
        qh = np.ascontiguousarray(self.qhat.numpy())
        out = np.empty(self.nv ** 3)
        rc = L.bfsm_emu_finish(ctypes.byref(d), fh.ctypes.data_as(dp), qh.ctypes.data_as(dp), out.ctypes.data_as(dp),
                               1 if with_loss else 0)
        if rc:
            raise RuntimeError(f"bfsm_emu_finish rc={rc}")
        Q.copy_(torch.from_numpy(out))


def collide_batch(fs, gl, sph, gamma, b_gamma, L, precision=64, max_chunk=0, flags=0, dir_range=(0, 0), gpu_groups=False,
                  max_batch=None):
    """fs: [n_batch][nvx][nvy][nvz]; one emulated bfsm_collide_batch call (on a direction shard: the shard's gain and the
    loss term) on a handle created for max_batch members (default: n_batch).  gpu_groups: as in collide.  Returns Q with the
    same shape."""
    fs = np.ascontiguousarray(fs, dtype=np.float64)
    nb = fs.shape[0]
    nv = fs.shape[1] if fs.shape[1] == fs.shape[2] == fs.shape[3] else fs.shape[1:]
    d, keep = make_desc(nv, gl, sph, gamma, b_gamma, L, precision, dir_range, max_chunk, flags, max_batch=max_batch or nb)
    L_ = lib_gpu_groups() if gpu_groups else lib()
    dp = ctypes.POINTER(ctypes.c_double)
    Q = np.empty_like(fs)
    rc = L_.bfsm_emu_collide_batch(ctypes.byref(d), fs.ctypes.data_as(dp), Q.ctypes.data_as(dp), None, nb)
    if rc:
        raise RuntimeError(f"bfsm_emu_collide_batch rc={rc}")
    return Q


class EmuOperatorFused(EmuOperator):
    """The same with collidePartial (the one-call form bfsm.sharded_step prefers when the operator offers it)."""

    def collidePartial(self, Q, f, with_loss, stream=0):
        import torch
        L = lib()
        dp = ctypes.POINTER(ctypes.c_double)
        d, keep = make_desc(self.nv, self.gl, self.sph, *self.args, 64, self.dir_range, self.max_chunk)
        fh = np.ascontiguousarray(f.numpy(), dtype=np.float64)
        out = np.empty(self.nv ** 3)
        rc = L.bfsm_emu_collide_partial(ctypes.byref(d), fh.ctypes.data_as(dp), out.ctypes.data_as(dp), 1 if with_loss else 0)
        if rc:
            raise RuntimeError(f"bfsm_emu_collide_partial rc={rc}")
        Q.copy_(torch.from_numpy(out))


def collide_partial(f, gl, sph, gamma, b_gamma, L, precision=64, dir_range=(0, 0), with_loss=True, flags=0, max_chunk=0):
    """Emulated bfsm_collide_partial_async (what bfsm_collide runs): at N = 16 the whole-direction kernels unless
    flags has BFSM_FLAG_NO_SMALL_PATH, otherwise the fused plane-tile sequence."""
    nv = f.shape[0] if f.shape[0] == f.shape[1] == f.shape[2] else f.shape
    d, keep = make_desc(nv, gl, sph, gamma, b_gamma, L, precision, dir_range, max_chunk, flags)
    f = np.ascontiguousarray(f, dtype=np.float64)
    Q = np.empty_like(f)
    dp = ctypes.POINTER(ctypes.c_double)
    L_ = lib()
    rc = L_.bfsm_emu_collide_partial(ctypes.byref(d), f.ctypes.data_as(dp), Q.ctypes.data_as(dp), 1 if with_loss else 0)
    if rc:
        raise RuntimeError(f"bfsm_emu_collide_partial rc={rc}")
    return Q


# entry points of bfsm_emu_gen_routes
ROUTE_OPS = {"collide": 0, "batch": 1, "partial": 2, "bilinear": 3, "fft_fwd": 4, "fft_bwd": 5}
# csrc/bfsm_generic.hpp enum class GK, in order
GK_NAMES = ("Fft", "Acc", "Combine", "FftBig", "Plane", "Line3", "PlaneAcc", "PlanePair", "Fft8", "FftBig8", "Line38")
# csrc/bfsm_generic.hpp load-side modes
GEN_MODES = {-1: None, 0: "PLAIN", 1: "PHASE", 2: "PRODUCT", 3: "REAL", 4: "BETA2", 5: "TAIL2"}


def gen_routes(shape, n_gl, n_sph, precision=64, op="collide", nb=1, max_chunk=0, dir_range=(0, 0), max_batch=0, gpu_groups=True):
    """Launches of one call of a size-generic entry point (op: a key of ROUTE_OPS), recorded by GenericPipeline's own host
    code with nothing executed and no scratch allocated.  gpu_groups: the GPU's plane-accumulate grouping (512 workgroups
    per launch, lib_gpu_groups) or the emulator's (24, lib).  Returns (launches, kernel_launches, info):
    launches = list of dicts (kind, precision, bilinear, mode, grid, lds, cat; and for the PlaneAcc / Acc launches groups =
    the slabs per member the launch writes / sums, mgroups = the distance between two members' slabs in arrays of G, n =
    the directions of the chunk, dir0 = its first direction), kernel_launches = the 6 per-category counts
    bfsm_get_counters reports under BFSM_FLAG_PROFILE, info = dict(together, gen_moves, plane, fused) of the pipeline
    (batch_together(), plan.gen_moves, plane_ok(), fused_ok()) plus what init allocated: slab_groups, chunk (directions
    resident at once), mb (members with scratch of their own), slab_arrays (the slab allocation in arrays of G) and chunks =
    [(first direction, length)] of the plan."""
    gl = (np.linspace(1.0, 2.0, n_gl), np.ones(n_gl))
    # nothing executes, so the rule's values do not matter: null vectors keep init's phase tables cheap (cos 0, sin 0)
    sph = (np.zeros(n_sph), np.zeros(n_sph), np.zeros(n_sph), np.ones(n_sph))
    d, keep = make_desc(tuple(shape), gl, sph, 0.0, 1.0, 11.0, precision, dir_range, max_chunk, 0, max_batch)
    cap, ccap = 4096, 1024
    rows = (ctypes.c_int * (12 * cap))()
    kl = (ctypes.c_int * 6)()
    info = (ctypes.c_int * 9)()
    crows = (ctypes.c_longlong * (2 * ccap))()
    n = (lib_gpu_groups() if gpu_groups else lib()).bfsm_emu_gen_routes(ctypes.byref(d), ROUTE_OPS[op], nb, rows, cap, kl, info,
                                                                        crows, ccap)
    if n < 0:
        raise ValueError(f"bfsm_emu_gen_routes rejected {shape} {precision} {op}: rc={-n}")
    assert n <= cap and info[8] <= ccap
    out = []
    for i in range(n):
        r = rows[12 * i:12 * i + 12]
        out.append(dict(kind=GK_NAMES[r[0]], precision=r[1], bilinear=bool(r[2]), mode=GEN_MODES[r[3]],
                        grid=(r[4], r[5]), lds=r[6], cat=r[7], groups=r[8], mgroups=r[9], n=r[10], dir0=r[11]))
    return out, tuple(kl), dict(together=bool(info[0]), gen_moves=info[1], plane=bool(info[2]), fused=bool(info[3]),
                                slab_groups=info[4], chunk=info[5], mb=info[6], slab_arrays=info[7],
                                chunks=[(crows[2 * i], crows[2 * i + 1]) for i in range(info[8])])
