"""HIPBoltzmannOperator -- Python mirror of BoltzmannOperator<CUDA_Backend> (Collisions/CUDABoltzmannOperator.hpp:44-131)
over the C-ABI.  Same life-cycle as the reference object: construct (no work), initialize(), then call it with DEVICE
arrays (torch CUDA tensors of float64) as often as needed.  Errors raise BfsmError (the reference prints and exits)."""
import ctypes

import numpy as np

from . import capi


def shard_range(n_dirs, rank, world):
    """Contiguous, balanced range of flattened quadrature directions b = r*M_sph + s owned by `rank`."""
    base, rem = divmod(n_dirs, world)
    begin = rank * base + min(rank, rem)
    return begin, begin + base + (1 if rank < rem else 0)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class HIPBoltzmannOperator:
    def __init__(self, gl_quadrature, spherical_quadrature, Nvx, Nvy, Nvz, gamma, b_gamma, L):
        self.gl_quadrature = gl_quadrature
        self.spherical_quadrature = spherical_quadrature
        self.Nvx, self.Nvy, self.Nvz = int(Nvx), int(Nvy), int(Nvz)
        self.gamma, self.b_gamma, self.L = float(gamma), float(b_gamma), float(L)
        self._precision = capi.BFSM_F64
        self._device = 0
        self._dir_range = (0, 0)
        self._max_chunk = 0
        self._flags = 0
        self._max_batch = 0
        self._h = None
        self._lib = None
        self._lin_tmp = None

    # knobs, to be set before initialize() -- like setWisdomFileName in the FFTW backend (FFTWBoltzmannOperator.hpp:39-41)
    def setPrecision(self, bits):
        self._precision = int(bits)

    def setDevice(self, ordinal):
        self._device = int(ordinal)

    def setDirectionShard(self, begin, end):
        self._dir_range = (int(begin), int(end))

    def setMaxChunk(self, n):
        self._max_chunk = int(n)

    def setMaxBatch(self, n):
        """Distributions per computeCollisionBatch call (scratch scales with it)."""
        self._max_batch = int(n)

    def setProfiling(self, on=True):
        self._flags = (self._flags | capi.BFSM_FLAG_PROFILE) if on else (self._flags & ~capi.BFSM_FLAG_PROFILE)

    def setExactReductions(self, on=True, hermitian=False):
        """Opt-in SURVEY 8(f1) reductions (antipodal pairs + one forward FFT per radial node); default off.
        hermitian=True adds BFSM_FLAG_HERMITIAN (only the lx >= 0 planes of A1', A2' are computed and stored)."""
        f = capi.BFSM_FLAG_EXACT_REDUCTIONS | capi.BFSM_FLAG_HERMITIAN
        self._flags &= ~f
        if on:
            self._flags |= capi.BFSM_FLAG_EXACT_REDUCTIONS | (capi.BFSM_FLAG_HERMITIAN if hermitian else 0)

    def setSmallPath(self, on=True):
        """N = 16: use (default) or avoid the whole-direction kernels for single evaluations (BFSM_FLAG_NO_SMALL_PATH)."""
        self._flags = (self._flags & ~capi.BFSM_FLAG_NO_SMALL_PATH) | (0 if on else capi.BFSM_FLAG_NO_SMALL_PATH)

    def setConservation(self, on=True):
        """Conservative projection of every Q this handle writes (BFSM_FLAG_CONSERVE): Q -> PQ with zero discrete mass,
        momentum and energy.  Default off."""
        self._flags = (self._flags | capi.BFSM_FLAG_CONSERVE) if on else (self._flags & ~capi.BFSM_FLAG_CONSERVE)

    def getBackendName(self):
        return (self._lib or capi.load_library()).bfsm_backend_name().decode()

    def _check(self, rc):
        if rc != capi.BFSM_OK:
            msg = self._lib.bfsm_last_error(self._h).decode() if self._lib else "?"
            raise capi.BfsmError(rc, msg)

    def initialize(self):
        self._lib = capi.load_library()
        gl, sp = self.gl_quadrature, self.spherical_quadrature
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in
                (gl.getNodes(), gl.getWeights(), sp.getWeights(), sp.getx(), sp.gety(), sp.getz())]
        dp = ctypes.POINTER(ctypes.c_double)
        d = capi.Desc(self.Nvx, self.Nvy, self.Nvz, gl.getNumberOfPoints(), sp.getNumberOfPoints(),
                      *[a.ctypes.data_as(dp) for a in keep],
                      self.gamma, self.b_gamma, self.L, self._precision, self._device,
                      self._dir_range[0], self._dir_range[1], self._max_chunk, self._flags, self._max_batch)
        h = ctypes.c_void_p()
        rc = self._lib.bfsm_create(ctypes.byref(d), ctypes.byref(h))
        if rc != capi.BFSM_OK:
            raise capi.BfsmError(rc, self._lib.bfsm_last_error(None).decode())
        self._h = h

    def _require(self, f, Q=None):
        if self._h is None:
            raise RuntimeError("initialize() has not been called")
        G = self.Nvx * self.Nvy * self.Nvz
        for t in (f, Q):
            if t is None:
                continue
            if not (t.is_cuda and t.dtype.is_floating_point and t.element_size() == 8 and t.is_contiguous() and t.numel() == G):
                raise ValueError("f and Q must be contiguous float64 CUDA tensors with Nvx*Nvy*Nvz elements")

    def computeCollision(self, Q, f_in):
        """Blocking evaluation, device tensors in and out (CUDABoltzmannOperator.cu:119-220)."""
        self._require(f_in, Q)
        self._check(self._lib.bfsm_collide(self._h, _ptr(Q), _ptr(f_in)))

    __call__ = computeCollision

    def computeCollisionAsync(self, Q, f_in, stream=0):
        self._require(f_in, Q)
        self._check(self._lib.bfsm_collide_async(self._h, _ptr(Q), _ptr(f_in), ctypes.c_void_p(stream)))

    def computeCollisionBatch(self, Q, f_in, n_batch, stream=None):
        """n_batch distributions [n_batch][Nvx*Nvy*Nvz] in one set of launches.  Blocking when
        stream is None, otherwise enqueued on that stream."""
        if self._h is None:
            raise RuntimeError("initialize() has not been called")
        G = self.Nvx * self.Nvy * self.Nvz
        for t in (f_in, Q):
            if not (t.is_cuda and t.element_size() == 8 and t.is_contiguous() and t.numel() == n_batch * G):
                raise ValueError("f and Q must be contiguous float64 CUDA tensors with n_batch*Nvx*Nvy*Nvz elements")
        if stream is None:
            self._check(self._lib.bfsm_collide_batch(self._h, _ptr(Q), _ptr(f_in), int(n_batch)))
        else:
            self._check(self._lib.bfsm_collide_batch_async(self._h, _ptr(Q), _ptr(f_in), int(n_batch),
                                                           ctypes.c_void_p(stream)))

    def collideBatchPartial(self, Q, f_in, n_batch, with_loss, stream=0):
        """Batch x direction shard: member i of Q = this shard's partial result for member i [- its loss term]; the
        caller sums Q over the ranks with one collective for the whole batch."""
        G = self.Nvx * self.Nvy * self.Nvz
        for t in (f_in, Q):
            if not (t.is_cuda and t.element_size() == 8 and t.is_contiguous() and t.numel() == n_batch * G):
                raise ValueError("f and Q must be contiguous float64 CUDA tensors with n_batch*Nvx*Nvy*Nvz elements")
        self._check(self._lib.bfsm_collide_batch_partial_async(self._h, _ptr(Q), _ptr(f_in), int(n_batch),
                                                               1 if with_loss else 0, ctypes.c_void_p(stream)))

    # Bilinear form Q(g,f) (include/bfsm.h): gain with A1 from g_hat and A2 from f_hat, loss g * Re IFFT(beta2 f_hat / G).
    # Q(f,f) is computeCollision; handles with exact reductions raise (BFSM_ERR_UNSUPPORTED).
    def computeBilinearCollision(self, Q, g, f):
        """Blocking Q = Q(g, f), device tensors."""
        self._require(g, Q)
        self._require(f)
        self._check(self._lib.bfsm_collide_bilinear(self._h, _ptr(Q), _ptr(g), _ptr(f)))

    def computeBilinearCollisionAsync(self, Q, g, f, stream=0):
        self._require(g, Q)
        self._require(f)
        self._check(self._lib.bfsm_collide_bilinear_async(self._h, _ptr(Q), _ptr(g), _ptr(f), ctypes.c_void_p(stream)))

    def collideBilinearPartial(self, Q, g, f, with_loss, stream=0):
        """This shard's part of Q(g, f) [- the loss term if with_loss]; the caller sums Q over the ranks."""
        self._require(g, Q)
        self._require(f)
        self._check(self._lib.bfsm_collide_bilinear_partial_async(self._h, _ptr(Q), _ptr(g), _ptr(f), 1 if with_loss else 0,
                                                                  ctypes.c_void_p(stream)))

    def linearizedCollision(self, Q, f, h, tmp=None):
        """Blocking Q = L_f[h] = Q(f, h) + Q(h, f), the Jacobian of Q at f applied to h (two bilinear evaluations).
        tmp: optional caller-owned device tensor of the same shape; otherwise a handle-owned one is allocated once."""
        self._require(f, Q)
        self._require(h)
        if tmp is None:
            if self._lin_tmp is None or self._lin_tmp.device != Q.device:
                self._lin_tmp = Q.new_empty(Q.shape)
            tmp = self._lin_tmp
        self._require(tmp)
        self.computeBilinearCollision(Q, f, h)
        self.computeBilinearCollision(tmp, h, f)
        Q.add_(tmp.view(Q.shape))

    # Symmetric form Qs(g, f) = Q(g, f) + Q(f, g) (include/bfsm.h, bfsm_collide_symmetric*): one call on ANY handle, the exact and
    # Hermitian modes included; L_f[h] = Qs(f, h), Qs(f, f) = 2 Q(f, f).
    def computeSymmetricCollision(self, Q, g, f):
        """Blocking Q = Q(g, f) + Q(f, g), device tensors; needs a handle that owns all directions."""
        self._require(g, Q)
        self._require(f)
        self._check(self._lib.bfsm_collide_symmetric(self._h, _ptr(Q), _ptr(g), _ptr(f)))

    def computeSymmetricCollisionAsync(self, Q, g, f, stream=0):
        self._require(g, Q)
        self._require(f)
        self._check(self._lib.bfsm_collide_symmetric_async(self._h, _ptr(Q), _ptr(g), _ptr(f), ctypes.c_void_p(stream)))

    def collideSymmetricPartial(self, Q, g, f, with_loss, stream=0):
        """This shard's part of Q(g, f) + Q(f, g) [- both loss terms if with_loss]; the caller sums Q over the ranks."""
        self._require(g, Q)
        self._require(f)
        self._check(self._lib.bfsm_collide_symmetric_partial_async(self._h, _ptr(Q), _ptr(g), _ptr(f), 1 if with_loss else 0,
                                                                   ctypes.c_void_p(stream)))

    # Gain / loss split (include/bfsm.h, bfsm_collide_split*): Qgain = the gain Q+, nu = the collision frequency nu[f], so that
    # Q = Qgain - f * nu (bilinear form: Qgain - g * nu).  BFSM_FLAG_CONSERVE has no effect on them.
    def _require_batch(self, n_batch, *tensors):
        if self._h is None:
            raise RuntimeError("initialize() has not been called")
        G = self.Nvx * self.Nvy * self.Nvz
        for t in tensors:
            if t is None:
                continue
            if not (t.is_cuda and t.dtype.is_floating_point and t.element_size() == 8 and t.is_contiguous()
                    and t.numel() == int(n_batch) * G):
                raise ValueError("arguments must be contiguous float64 CUDA tensors with n_batch*Nvx*Nvy*Nvz elements")

    # Batched two-operand forms (include/bfsm.h, bfsm_collide_symmetric_batch*, bfsm_collide_bilinear_batch_partial_async): member i
    # of Q = Qs(g_i, f_i) or Q(g_i, f_i) for n_batch <= max_batch pairs in one launch sequence.  share: None, "g" or "f" -- that
    # operand is ONE distribution (G elements) every member uses, transformed once.
    def _require_pairs(self, Q, g, f, n_batch, share):
        if share not in capi.SHARE:
            raise ValueError('share must be None, "g" or "f"')
        self._require_batch(n_batch, Q)
        self._require_batch(1 if share == "g" else n_batch, g)
        self._require_batch(1 if share == "f" else n_batch, f)
        return capi.SHARE[share]

    def computeSymmetricCollisionBatch(self, Q, g, f, n_batch, share=None, stream=None):
        """Q[i] = Qs(g_i, f_i); needs a handle that owns all directions.  stream=None: blocking; otherwise enqueued on it."""
        sh = self._require_pairs(Q, g, f, n_batch, share)
        if stream is None:
            self._check(self._lib.bfsm_collide_symmetric_batch(self._h, _ptr(Q), _ptr(g), _ptr(f), int(n_batch), sh))
            return
        n_dirs = self.gl_quadrature.getNumberOfPoints() * self.spherical_quadrature.getNumberOfPoints()
        if self._dir_range not in ((0, 0), (0, n_dirs)):
            raise ValueError("computeSymmetricCollisionBatch needs a handle that owns all directions; use collideSymmetricBatchPartial")
        self.collideSymmetricBatchPartial(Q, g, f, n_batch, True, share, stream)

    def collideSymmetricBatchPartial(self, Q, g, f, n_batch, with_loss, share=None, stream=0):
        """This shard's part of Qs(g_i, f_i) [- both loss terms if with_loss] for every member; the caller sums Q over the ranks."""
        sh = self._require_pairs(Q, g, f, n_batch, share)
        self._check(self._lib.bfsm_collide_symmetric_batch_partial_async(self._h, _ptr(Q), _ptr(g), _ptr(f), int(n_batch), sh,
                                                                         1 if with_loss else 0, ctypes.c_void_p(stream)))

    def collideBilinearBatchPartial(self, Q, g, f, n_batch, with_loss, share=None, stream=0):
        """This shard's part of Q(g_i, f_i) [- the loss term if with_loss] for every member; faithful handles only."""
        sh = self._require_pairs(Q, g, f, n_batch, share)
        self._check(self._lib.bfsm_collide_bilinear_batch_partial_async(self._h, _ptr(Q), _ptr(g), _ptr(f), int(n_batch), sh,
                                                                        1 if with_loss else 0, ctypes.c_void_p(stream)))

    def computeCollisionSplit(self, Qgain, nu, f_in):
        """Blocking Qgain = Q+(f,f), nu = nu[f], device tensors; needs a handle that owns all directions."""
        self._require_batch(1, Qgain, nu, f_in)
        self._check(self._lib.bfsm_collide_split(self._h, _ptr(Qgain), _ptr(nu), _ptr(f_in)))

    def computeCollisionSplitAsync(self, Qgain, nu, f_in, stream=0):
        self._require_batch(1, Qgain, nu, f_in)
        self._check(self._lib.bfsm_collide_split_async(self._h, _ptr(Qgain), _ptr(nu), _ptr(f_in), ctypes.c_void_p(stream)))

    def collideSplitBatchPartial(self, Qgain, nu, f_in, n_batch, with_loss, stream=0):
        """Batch x direction shard: member i of Qgain = this shard's part of the gain of member i (the caller sums it over the
        ranks); nu (written only if with_loss, otherwise it may be None) = nu[f_i]."""
        self._require_batch(n_batch, Qgain, nu, f_in)
        if with_loss and nu is None:
            raise ValueError("nu may be None only with with_loss = False")
        self._check(self._lib.bfsm_collide_split_batch_partial_async(
            self._h, _ptr(Qgain), _ptr(nu) if nu is not None else None, _ptr(f_in), int(n_batch), 1 if with_loss else 0,
            ctypes.c_void_p(stream)))

    def collideBilinearSplitPartial(self, Qgain, nu, g, f, with_loss, stream=0):
        """This shard's part of the gain of Q(g, f) and, if with_loss, nu = nu[f] (else nu may be None)."""
        self._require_batch(1, Qgain, nu, g, f)
        if with_loss and nu is None:
            raise ValueError("nu may be None only with with_loss = False")
        self._check(self._lib.bfsm_collide_bilinear_split_partial_async(
            self._h, _ptr(Qgain), _ptr(nu) if nu is not None else None, _ptr(g), _ptr(f), 1 if with_loss else 0,
            ctypes.c_void_p(stream)))

    def computeBilinearSplit(self, Qgain, nu, g, f):
        """Blocking Qgain = Q+(g, f), nu = nu[f]: Q(g, f) = Qgain - g * nu; needs a handle that owns all directions."""
        n_dirs = self.gl_quadrature.getNumberOfPoints() * self.spherical_quadrature.getNumberOfPoints()
        if self._dir_range not in ((0, 0), (0, n_dirs)):
            raise ValueError("computeBilinearSplit needs a handle that owns all directions; use collideBilinearSplitPartial")
        self.collideBilinearSplitPartial(Qgain, nu, g, f, True)
        self.synchronize()

    def lossRate(self, nu, f_in, n_batch=1, stream=0):
        """nu = nu[f] = Re IFFT(beta2 f_hat / G) for n_batch distributions, no gain work; any handle; enqueued on `stream`."""
        self._require_batch(n_batch, nu, f_in)
        self._check(self._lib.bfsm_loss_rate_async(self._h, _ptr(nu), _ptr(f_in), int(n_batch), ctypes.c_void_p(stream)))

    def gainPartial(self, f_in, stream=0):
        self._require(f_in)
        self._check(self._lib.bfsm_gain_partial(self._h, _ptr(f_in), ctypes.c_void_p(stream)))

    def finish(self, Q, f_in, stream=0):
        self._require(f_in, Q)
        self._check(self._lib.bfsm_finish(self._h, _ptr(Q), _ptr(f_in), ctypes.c_void_p(stream)))

    def finishPartial(self, Q, f_in, with_loss, stream=0):
        """Q = Re IFFT(this shard's partial Q_gain_hat) [- loss term if with_loss]; the caller sums Q over ranks."""
        self._require(f_in, Q)
        self._check(self._lib.bfsm_finish_partial(self._h, _ptr(Q), _ptr(f_in), 1 if with_loss else 0,
                                                  ctypes.c_void_p(stream)))

    def collidePartial(self, Q, f_in, with_loss, stream=0):
        """gainPartial + finishPartial as one call (slab reduce fused into the tail; qhatBuffer() is not updated)."""
        self._require(f_in, Q)
        self._check(self._lib.bfsm_collide_partial_async(self._h, _ptr(Q), _ptr(f_in), 1 if with_loss else 0,
                                                         ctypes.c_void_p(stream)))

    def conserve(self, Q, n_batch=1, stream=0):
        """Q := PQ in place for n_batch consecutive distributions (bfsm_conserve_async; any handle, flag or not), enqueued on
        `stream`."""
        if self._h is None:
            raise RuntimeError("initialize() has not been called")
        G = self.Nvx * self.Nvy * self.Nvz
        if not (Q.is_cuda and Q.element_size() == 8 and Q.is_contiguous() and Q.numel() == int(n_batch) * G):
            raise ValueError("Q must be a contiguous float64 CUDA tensor with n_batch*Nvx*Nvy*Nvz elements")
        self._check(self._lib.bfsm_conserve_async(self._h, _ptr(Q), int(n_batch), ctypes.c_void_p(stream)))

    # Macroscopic state of f and its Maxwellian (include/bfsm.h, bfsm_moments_async / bfsm_maxwellian_async): rows of
    # capi.MOM_COUNT doubles (capi.MOM_RHO ... capi.MOM_H) in device memory, so moments -> maxwellian needs no host round trip.
    def _require_rows(self, mom, n_batch):
        if not (mom.is_cuda and mom.dtype.is_floating_point and mom.element_size() == 8 and mom.is_contiguous()
                and mom.numel() == int(n_batch) * capi.MOM_COUNT):
            raise ValueError("mom must be a contiguous float64 CUDA tensor with n_batch*MOM_COUNT elements")

    def moments(self, mom, f, n_batch=1, stream=0):
        """mom[i] = (rho, m, E, u, T, H) of f[i] for n_batch distributions; any handle; enqueued on `stream`."""
        self._require_batch(n_batch, f)
        self._require_rows(mom, n_batch)
        self._check(self._lib.bfsm_moments_async(self._h, _ptr(mom), _ptr(f), int(n_batch), ctypes.c_void_p(stream)))

    def maxwellian(self, M, mom, n_batch=1, stream=0):
        """M[i] = the Maxwellian of rho, u, T of row mom[i] on the grid (0 where rho or T is not finite and positive); any
        handle; enqueued on `stream`."""
        self._require_batch(n_batch, M)
        self._require_rows(mom, n_batch)
        self._check(self._lib.bfsm_maxwellian_async(self._h, _ptr(M), _ptr(mom), int(n_batch), ctypes.c_void_p(stream)))

    def qhatBuffer(self):
        """(device pointer, n_elems, precision) of the partial Q_gain_hat owned by the handle."""
        n = ctypes.c_size_t()
        prec = ctypes.c_int()
        p = self._lib.bfsm_qhat_buffer(self._h, ctypes.byref(n), ctypes.byref(prec))
        return p, n.value, prec.value

    def synchronize(self):
        self._check(self._lib.bfsm_synchronize(self._h))

    def fft3d(self, data, batch, sign):
        self._check(self._lib.bfsm_fft3d(self._h, _ptr(data), int(batch), int(sign)))

    def counters(self):
        c = capi.Counters()
        self._check(self._lib.bfsm_get_counters(self._h, ctypes.byref(c)))
        return c

    def destroy(self):
        if self._h is not None and self._lib is not None:
            self._lib.bfsm_destroy(self._h)
        self._h = None
        self._lin_tmp = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
