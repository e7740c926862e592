/*
 * bfsm.h -- C-ABI of the MI355X-native Fourier-spectral Boltzmann collision operator (libbfsm_hip.so).
 *
 * This is the drop-in boundary for ONE path of i3s93/Boltzmann-Fourier-Spectral-Method: a single evaluation of
 * Q = Q(f,f) behind AbstractCollisionOperator::computeCollision.  Plain pointers and sizes only; no C++ or torch
 * types.  Each entry point names the reference interface it replaces (file:line relative to the reference root).
 * The C++ mirror of the reference's operator class (BoltzmannOperator<HIP_Backend>) and the Python ctypes binding
 * are thin wrappers over exactly these symbols; see INTEGRATION.md.
 *
 * Conventions (identical to the reference's CUDA backend, Collisions/CUDABoltzmannOperator.cu:119-220):
 *   - f and Q are DEVICE pointers to Nvx*Nvy*Nvz contiguous doubles, row-major [i][j][k], k (v_z) contiguous
 *     (maxwell_bkw_cuda.cu:119-126); they stay owned by the caller, all scratch is owned by the handle.
 *   - a handle is not re-entrant (shared scratch), like the reference object: one thread at a time per handle, and
 *     consecutive calls on one handle must be ordered on the device (same stream, or the caller's own events) because
 *     they reuse the scratch.  Different handles are independent and may be driven from different threads / streams.
 *   - every call makes the handle's device current for its own duration and restores the calling thread's current
 *     device before it returns.
 *   - the *_async entry points only enqueue kernels on the given stream: no allocation and no synchronisation after the
 *     first evaluation; per call one host-side capture-status query (hipStreamIsCapturing) and, outside a capture, one
 *     record of a handle-owned event behind the call's work (what bfsm_synchronize waits for; the event of a stream is
 *     created at its first use).  After one evaluation outside a capture they can therefore be captured into a HIP graph;
 *     nothing is recorded during a capture, so replays of such a graph are the caller's to synchronise.  The caller's
 *     stream handle is never used after the call returns: the caller may destroy the stream at any time (a NEW stream
 *     that reuses the handle value of a destroyed one takes over its entry: bfsm_synchronize then covers the new
 *     stream's work; the destroyed stream's work completes under hipStreamDestroy's own rules).
 *   - functions never throw and never exit: they return BFSM_OK or an error code, and bfsm_last_error() returns a
 *     human-readable message (the reference prints and std::exit()s, CUDABoltzmannOperator.hpp:20-38; the C++
 *     wrapper restores that behaviour).
 */
#ifndef BFSM_H
#define BFSM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFSM_VERSION 2   /* 2: any-box grids, bfsm_collide_batch_partial_async, BFSM_FLAG_NO_SMALL_PATH */

enum {
    BFSM_OK = 0,
    BFSM_ERR_INVALID = 1,      /* bad argument / descriptor */
    BFSM_ERR_UNSUPPORTED = 2,  /* grid size / precision combination without a kernel */
    BFSM_ERR_HIP = 3,          /* a HIP runtime call failed (message has file:line) */
    BFSM_ERR_NOMEM = 4
};

enum {
    BFSM_F64 = 64, /* IEEE double throughout (reference behaviour) */
    BFSM_F32 = 32  /* single-precision transforms and tables; f and Q stay double at the boundary */
};

enum {
    BFSM_FLAG_NONE = 0,
    BFSM_FLAG_PROFILE = 1, /* record HIP events around every kernel launch (bfsm_get_counters) */
    /* Opt-in exact work reductions; results equal the faithful path up to rounding order (~1e-16):
     *  (i)  antipodal pairs: if the spherical rule satisfies sigma_{s+M/2} == -sigma_s with equal weights (all shipped
     *       symmetric designs do, bit-exactly), direction s+M/2 gives the same product A1*A2 as s, so only M/2
     *       directions per radial node are evaluated, with doubled weight; otherwise this part is skipped;
     *  (ii) FFT linearity: the products of all directions of a radial node are summed in physical space and
     *       forward-transformed once, instead of one forward FFT per direction.
     * The default (flag clear) evaluates every direction: its own two inverse 3-D transforms, its own product and the
     * x part of its own forward transform; the (y,z) part of the forward transform is applied once to the weighted sum
     * of a run of directions that share a radial node (linearity).  That sum is formed in registers by the kernel that
     * runs the x transforms, so the half-transformed product of a direction is never written: A1' and A2' are written
     * and read once per direction, the sum once per run -- 4 array passes per direction + 4 per run, DESIGN.md section 4.
     * On boxes served by the size-generic path (see bfsm_desc::nvx) this flag and BFSM_FLAG_HERMITIAN are accepted and
     * have no effect (the results are the same by definition; bfsm_counters::exact_reductions reports 0). */
    BFSM_FLAG_EXACT_REDUCTIONS = 2,
    /* Additional exact reduction on top of BFSM_FLAG_EXACT_REDUCTIONS (invalid without it): f is real, so the
     * half-transformed arrays satisfy A'[-lx] = conj A'[lx] up to the three Nyquist planes; only the planes
     * lx = 0 .. N/2 are computed and stored, the rest is rebuilt by conjugation plus exact rank-one Nyquist terms
     * (the r2c / c2r saving the reference lists as future work, CUDABoltzmannOperator.cu:36). */
    BFSM_FLAG_HERMITIAN = 4,
    /* N = 16 only: do not use the whole-direction kernels (a direction kept in one workgroup's LDS, two launches
     * per evaluation) for single evaluations; the plane-tile pipeline of the larger grids is used instead.  Same
     * results up to rounding order; for comparisons and tests. */
    BFSM_FLAG_NO_SMALL_PATH = 8,
    /* Conservative spectral method (Gamba & Tharkabhushanam, J. Comput. Phys. 2009; new functionality, INTEGRATION.md
     * section 6): every entry point that writes Q writes PQ instead -- bfsm_collide*, bfsm_collide_batch*, bfsm_finish,
     * bfsm_finish_partial, bfsm_collide_partial_async, bfsm_collide_batch_partial_async, bfsm_collide_bilinear* and bfsm_collide_symmetric*.  P is the
     * L2-orthogonal projection onto the grid functions with zero discrete mass, momentum and energy:
     *     PQ = Q - sum_k (<psi_k, Q> / <psi_k, psi_k>) psi_k,   psi = {1, vx, vy, vz, |v|^2 - c},  c = mean of |v|^2 over the grid,
     * <a,b> = sum over the G grid points (the grid is symmetric on every axis, so the basis is orthogonal).  P is fixed and
     * linear: on the partial forms it is applied to each rank's share and the caller's sum is P of the whole Q; batches are
     * projected member by member.  Always computed in fp64 (also on BFSM_F32 handles), bitwise reproducible, allocation-free.
     * Combines with the exact / Hermitian modes and the N = 16 path.  bfsm_qhat_buffer() (spectral, before the finish) is not
     * projected.  For the bilinear form P is applied to Q(g,f) itself: Q(g,f) alone conserves only mass in the continuum,
     * so PQ(g,f) is the part of Q(g,f) orthogonal to the invariants, and the symmetric sum L_f[h] = PQ(f,h) + PQ(h,f) is
     * exactly P of the linearized operator (the Jacobian of P o Q).  Q must be 16-byte aligned (BFSM_ERR_INVALID otherwise).
     * Libraries without this feature ignore the bit: the presence of bfsm_conserve_async is the capability check. */
    BFSM_FLAG_CONSERVE = 16
};

typedef struct bfsm_plan* bfsm_handle;

/*
 * Operator description == the constructor arguments of BoltzmannOperator<CUDA_Backend>
 * (Collisions/CUDABoltzmannOperator.hpp:48-54) with the quadrature objects flattened to the arrays the operator
 * reads from them (getNodes/getWeights, Quadratures/AbstractQuadrature.hpp:17-29; getx/gety/getz/getWeights,
 * Quadratures/AbstractSphericalQuadratures.hpp:21-42).  All arrays are HOST pointers, copied during create.
 */
typedef struct bfsm_desc {
    int nvx, nvy, nvz;        /* velocity grid: every extent even, in [4, 256], prime factors 2, 3, 5, 7, 11, 13 (the
                                 reference plans any Nvx x Nvy x Nvz, CUDABoltzmannOperator.cu:86-100).  Cubes of 16, 24, 32,
                                 40, 48, 64, 80, 96, 128 run on the fused pipeline (4 array passes per direction); every other box
                                 on the size-generic path (run-time sizes: the same three fused kernels where a (y,z) plane
                                 fits the LDS, per-axis passes otherwise; a half to a sixth of the fused pipeline's speed),
                                 both precisions.  Anything else: BFSM_ERR_UNSUPPORTED */
    int n_gl;                 /* Gauss-Legendre points (radial)          */
    int n_sph;                /* spherical quadrature points             */
    const double* gl_nodes;   /* [n_gl]  rho_r on [0,R]                   */
    const double* gl_wts;     /* [n_gl]                                   */
    const double* sph_wts;    /* [n_sph]                                  */
    const double* sx;         /* [n_sph] unit vectors                     */
    const double* sy;
    const double* sz;
    double gamma;             /* kernel exponent (0: Maxwell molecules)   */
    double b_gamma;           /* kernel constant                          */
    double L;                 /* half-width of the periodic velocity box  */
    int precision;            /* BFSM_F64 | BFSM_F32                      */
    int device;               /* HIP device ordinal                       */
    long long dir_begin;      /* shard of the flattened quadrature directions b = r*n_sph + s handled by this   */
    long long dir_end;        /* handle: [dir_begin, dir_end).  0,0 = all directions (single-GPU behaviour).     */
    int max_chunk;            /* directions resident at once (0 = default: 1024 on the fused cubes, 256 on the size-
                                 generic path: the whole shard in one pass when it fits; scratch = 2 * chunk * G
                                 complex); bounds scratch, not results                                               */
    int flags;                /* BFSM_FLAG_*                              */
    int max_batch;            /* distributions per bfsm_collide_batch call (0/1 = single); scratch scales with it */
} bfsm_desc;

/* Per-kernel accounting filled when BFSM_FLAG_PROFILE is set (all zero otherwise). */
enum { BFSM_K_FFT_F = 0, BFSM_K_GAIN_INV = 1, BFSM_K_GAIN_LINE = 2, BFSM_K_GAIN_FWD = 3, BFSM_K_REDUCE = 4,
       BFSM_K_TAIL = 5, BFSM_K_COUNT = 6 };
typedef struct bfsm_counters {
    double alg_bytes_per_eval;            /* (6*B_shard + 9) * G * c, the SURVEY 8(d) model                 */
    double kernel_ms[BFSM_K_COUNT];       /* summed HIP-event time of the last profiled evaluation         */
    double kernel_alg_bytes[BFSM_K_COUNT];/* algorithmic bytes moved by those launches                     */
    int kernel_launches[BFSM_K_COUNT];
    int n_chunks;
    int chunk_dirs;                       /* directions in the largest chunk                               */
    long long n_dirs;                     /* work units of this shard (directions; antipodal pairs if merged) */
    double moved_bytes_per_eval;          /* bytes the launch sequence moves (model): (4*n_dirs + 4*segments + 9) * G * c
                                             on the fused pipeline (n_dirs: work units of the mode), i.e. LESS than
                                             alg_bytes_per_eval, the reference model of three transforms per direction */
    int exact_reductions;                 /* 1 if the flag is active                                          */
    int antipodal_merged;                 /* 1 if antipodal pairs were merged                                 */
} bfsm_counters;

/* == BoltzmannOperator<CUDA_Backend>::initialize() (CUDABoltzmannOperator.cu:28-115): allocates all device
 * scratch, uploads quadrature-derived tables, builds twiddles.  Returns a handle through *out. */
int bfsm_create(const bfsm_desc* desc, bfsm_handle* out);

/* == BoltzmannOperator<CUDA_Backend>::computeCollision(Q, f_in) (CUDABoltzmannOperator.cu:119-220), blocking:
 * returns after the device work has completed (the reference ends in cudaDeviceSynchronize, cu:218).
 * Requires a handle that owns ALL directions (dir_begin,dir_end = 0,0 or 0,n_gl*n_sph). */
int bfsm_collide(bfsm_handle h, double* Q_dev, const double* f_dev);

/* Same, enqueued on `stream` (a hipStream_t cast to void*; NULL = the device's legacy default stream, which is what
 * the reference launches on, cu:131-218) without the final host synchronisation. */
int bfsm_collide_async(bfsm_handle h, double* Q_dev, const double* f_dev, void* stream);

/* Batch of distributions (new functionality): f_dev and Q_dev hold n_batch <= desc.max_batch
 * consecutive N^3 arrays; every kernel launch covers the whole batch (one more grid dimension), so the quadrature
 * tables are shared and small grids (N = 16, 32) fill the GPU.  Member i of the result is bitwise identical to
 * bfsm_collide on member i alone ON THE SAME HANDLE (a handle created with max_batch > 1 keeps one set of kernels for
 * single and batched calls; a batch of one on a max_batch <= 1 handle is bfsm_collide itself).  Batches are
 * independent: on several GPUs they shard without any collective. */
int bfsm_collide_batch(bfsm_handle h, double* Q_dev, const double* f_dev, int n_batch);
int bfsm_collide_batch_async(bfsm_handle h, double* Q_dev, const double* f_dev, int n_batch, void* stream);
/* Batch x direction shard in one call (the two data-parallel axes composed): the handle may own any shard of the
 * directions; member i of Q_dev receives Re IFFT(this shard's partial Q_gain_hat of member i) [- loss term of member i
 * if with_loss].  The caller sums Q_dev (n_batch * G doubles) over the ranks with ONE collective for the whole batch;
 * exactly one rank passes with_loss != 0.  bfsm_collide_batch_async == this with all directions and with_loss = 1. */
int bfsm_collide_batch_partial_async(bfsm_handle h, double* Q_dev, const double* f_dev, int n_batch, int with_loss,
                                     void* stream);

/*
 * Sharded evaluation (new functionality: the reference is single-device).  Every rank calls
 *   bfsm_gain_partial()  -> this shard's partial Q_gain_hat in the handle-owned buffer bfsm_qhat_buffer()
 *   <one sum all-reduce / reduce of that buffer: RCCL over xGMI, by the caller>
 *   bfsm_finish()        -> loss term, final inverse transforms, Q        (cu:193-216)
 * bfsm_collide() == gain_partial + finish on one device.
 */
int bfsm_gain_partial(bfsm_handle h, const double* f_dev, void* stream);
int bfsm_finish(bfsm_handle h, double* Q_dev, const double* f_dev, void* stream);
/* Cheaper sharded route (half the bytes on the wire, nothing after the collective): the inverse transform is linear,
 * so every rank transforms its OWN partial Q_gain_hat and the caller sums the real results:
 *   bfsm_gain_partial()
 *   bfsm_finish_partial(h, Q, f, with_loss = (rank == 0), stream)   -> Q = Re IFFT(partial Q_gain_hat) [- loss term]
 *   <one sum all-reduce of Q (G doubles), by the caller>
 * Exactly one rank passes with_loss != 0. */
int bfsm_finish_partial(bfsm_handle h, double* Q_dev, const double* f_dev, int with_loss, void* stream);
/* The same two steps as ONE call, which lets the library fuse the slab reduce into the first tail kernel when the
 * shard has few slabs (one launch and one pass over Q_hat fewer; bitwise the same Q).  The contents of
 * bfsm_qhat_buffer() are unspecified after this call and after bfsm_collide / bfsm_collide_batch, which are this
 * sequence with with_loss = 1; only bfsm_gain_partial defines them. */
int bfsm_collide_partial_async(bfsm_handle h, double* Q_dev, const double* f_dev, int with_loss, void* stream);
/* Device pointer to the (partial) Q_gain_hat: n_elems reals of `precision` bits (2*G, interleaved complex in the
 * library's spectral layout [lx][lz][ly]); the buffer the collective must sum in place. */
void* bfsm_qhat_buffer(bfsm_handle h, size_t* n_elems, int* precision);

/*
 * Bilinear form Q(g,f) (new functionality; the presence of these symbols is the capability check, BFSM_VERSION stays 2).
 * The oracle loop with three changes: A1 is formed from g_hat = FFT(g), A2 from f_hat = FFT(f) (same phase factors as in
 * Q(f,f)), and the loss is multiplied by g:
 *     Q(g,f) = Re IFFT(Q_gain_hat[g_hat, f_hat]) - g * Re IFFT(beta2 f_hat / G).
 * Q(f,f) is the operator of bfsm_collide; Q is linear in each argument; the loss g(v) (beta2 * f)(v) is the rate at which
 * g-particles at v are scattered by f.  The linearized operator is L_f[h] = Q(f,h) + Q(h,f).  For a rule with
 * sigma_{s+M/2} == -sigma_s and equal weights (every shipped design) the gain is symmetric in (g,f); for other rules it is
 * not, and the definition above is what holds.
 *   - g, f, Q: device pointers to one distribution each (n_batch = 1).  g == f (the same pointer) is allowed; Q must not
 *     overlap g or f (BFSM_ERR_INVALID).
 *   - handles with BFSM_FLAG_EXACT_REDUCTIONS (and therefore BFSM_FLAG_HERMITIAN) return BFSM_ERR_UNSUPPORTED and leave Q
 *     untouched: their antipodal merge assumes g = f.
 *   - N = 16 handles evaluate it on the plane-tile pipeline (as with BFSM_FLAG_NO_SMALL_PATH): the whole-direction kernels
 *     have no room for a second cube.
 *   - the scratch is reserved at bfsm_create (two spectra), so the async forms are allocation-free and can be captured
 *     into a HIP graph after one evaluation outside a capture, like bfsm_collide_async.
 * bfsm_collide_bilinear is blocking; _async enqueues on `stream`; _partial_async works on a direction shard like
 * bfsm_collide_partial_async: Q = Re IFFT(this shard's partial gain) [- loss if with_loss], summed over the ranks by the
 * caller, exactly one rank passing with_loss != 0.
 */
int bfsm_collide_bilinear(bfsm_handle h, double* Q_dev, const double* g_dev, const double* f_dev);
int bfsm_collide_bilinear_async(bfsm_handle h, double* Q_dev, const double* g_dev, const double* f_dev, void* stream);
int bfsm_collide_bilinear_partial_async(bfsm_handle h, double* Q_dev, const double* g_dev, const double* f_dev,
                                        int with_loss, void* stream);

/*
 * Symmetric bilinear form (new functionality; the presence of these symbols is the capability check, BFSM_VERSION stays 2):
 *     Qs(g,f) = Q(g,f) + Q(f,g) = Re IFFT(Q_gain_hat[g_hat, f_hat] + Q_gain_hat[f_hat, g_hat]) - g * nu[f] - f * nu[g],
 * with Q(.,.) as above and nu[f] = Re IFFT(beta2 f_hat / G); the definition holds for any rule.  L_f[h] = Qs(f,h) and
 * Qs(f,f) = 2 Q(f,f).  Unlike Q(g,f) alone it is served by EVERY handle, the exact and Hermitian modes included: with
 * P_s(g,f) = IFFT(alpha_s g_hat) * IFFT(conj(alpha_s) f_hat) and alpha_{-sigma} = conj(alpha_sigma), P_{-sigma}(g,f) = P_sigma(f,g),
 * so on a rule with sigma_{s+M/2} == -sigma_s and equal weights (verified bit-exactly at bfsm_create)
 *     gain(g,f) + gain(f,g) = sum_{s < M/2} 2 w_s [P_s(g,f) + P_s(f,g)]:
 * the merged plan (M/2 directions, doubled weights) applied to both operand orders.  Both operand orders are computed for
 * every direction on every handle, so rules without that symmetry are served as well (unmerged, every direction twice).
 *   - g, f, Q: device pointers to one distribution each; a handle created with max_batch > 1 serves a single call (batches of
 *     pairs: bfsm_collide_symmetric_batch* below).  g == f
 *     (the same pointer) is allowed; Q must not overlap g or f (BFSM_ERR_INVALID); a null pointer gives BFSM_ERR_INVALID.
 *   - routes.  Fused cubes, every mode and both precisions: per chunk two passes of the gain kernels with the spectra
 *     exchanged -- KA (the bilinear operand selection, in the Hermitian mode with planes = N/2 + 1, its two-array form at
 *     N = 128 fp32 and its Nyquist-row guests at N = 64), the mode's own x-line kernel -- the second pass into segment sums
 *     and slabs of its own (buffers of this call alone, 2 x the plan's slabs, reserved at create); then ONE forward-tile pass, ONE reduce (fused into the
 *     tail when there are at most 8 slabs in all) and ONE tail with a third plane (beta2 g_hat) and the combine
 *     Q = gain - g nu[f] - f nu[g].  Four stored A' arrays per effective direction, written once and read once; fixed-order
 *     sums, no atomics, bitwise reproducible.  No geometry stores all N planes: the Hermitian saving applies everywhere.
 *     N = 16 takes the plane-tile pipeline, as for the bilinear form.  Size-generic boxes: the bilinear gain launches twice,
 *     the second pass accumulating onto the first one's Q_hat, then one tail with both loss terms (a second loss array in the
 *     idle A1 / A2 scratch, one combine kernel).
 *   - bfsm_collide_symmetric is blocking; _async enqueues on `stream`; both need a handle that owns all directions.
 *     _partial_async works on a direction shard: Q = Re IFFT(this shard's share of the symmetric gain) [- g nu[f] - f nu[g] if
 *     with_loss]; the caller sums Q over the ranks, exactly one rank passing with_loss != 0.  On merged handles the shard
 *     maps to effective directions exactly as for Q(f,f).
 *   - BFSM_FLAG_CONSERVE: Q := P Qs, applied once (Q 16-byte aligned, as on the other entry points).  P Qs(f,h) is exactly the
 *     Jacobian of P o Q at f applied to h.
 *   - the _async forms are allocation-free after bfsm_create, graph-capturable after one evaluation outside a capture and
 *     tracked by bfsm_synchronize.  With BFSM_FLAG_PROFILE the counters' kernel_launches / kernel_ms / kernel_alg_bytes cover
 *     the sequence (byte model: symmetric_moved_bytes_per_eval in csrc/bfsm_calls.hpp).
 *   - bfsm_collide_bilinear* and bfsm_collide_bilinear_split* are unchanged: BFSM_ERR_UNSUPPORTED on exact-reduction handles.
 */
int bfsm_collide_symmetric(bfsm_handle h, double* Q_dev, const double* g_dev, const double* f_dev);
int bfsm_collide_symmetric_async(bfsm_handle h, double* Q_dev, const double* g_dev, const double* f_dev, void* stream);
int bfsm_collide_symmetric_partial_async(bfsm_handle h, double* Q_dev, const double* g_dev, const double* f_dev,
                                         int with_loss, void* stream);

/*
 * Batched two-operand forms (new functionality; the presence of these symbols is the capability check, BFSM_VERSION stays 2):
 * member i of Q is Qs(g_i, f_i) (bfsm_collide_symmetric_batch*) or Q(g_i, f_i) (bfsm_collide_bilinear_batch_partial_async) for
 * n_batch pairs in ONE launch sequence -- what a Newton-Krylov or linearized-implicit step of a spatially inhomogeneous problem
 * applies in every cell, L_{f_i}[h_i] = Qs(f_i, h_i), and what a block Krylov method, Jacobian probing or a two-species cross
 * term applies to many h_i with one shared f, Qs(f, h_i).
 *   - Q is [n_batch][G], 1 <= n_batch <= max_batch of the descriptor.  An operand that is not shared is [n_batch][G].  With
 *     share = BFSM_SHARE_G (BFSM_SHARE_F), g (f) is ONE array of G doubles used by every member: member i of Q is Qs(g, f_i)
 *     (Qs(g_i, f)), likewise Q(.,.).  g == f as the same pointer with BFSM_SHARE_NONE is allowed and gives 2 Q(f_i, f_i).
 *     Q must not overlap any array that is read.  A null pointer, a bad n_batch or a bad share: BFSM_ERR_INVALID, nothing written.
 *   - the symmetric forms run on every handle (faithful, exact, Hermitian, both precisions, N = 16 on the plane-tile pipeline,
 *     size-generic boxes, direction shards: exactly one rank passes with_loss != 0, as for the single call).  The bilinear form
 *     returns BFSM_ERR_UNSUPPORTED on exact-reduction handles and leaves Q untouched, like bfsm_collide_bilinear*.
 *   - member i is bitwise bfsm_collide_symmetric_partial_async / bfsm_collide_bilinear_partial_async on member i's operands ON THE
 *     SAME HANDLE; it does not depend on n_batch, on share or on what the other members hold; repeated calls are bitwise
 *     identical (fixed-order sums, no atomics).  BFSM_FLAG_CONSERVE projects every member (Q 16-byte aligned).
 *   - fused cubes: two spectra passes, then per chunk the two gain passes with the batch in the grid, one forward-tile pass, one
 *     reduce (fused into the tail when 2 x slabs <= 8), one three-plane tail; with n_batch = 1 the launches of the single call.  A
 *     shared operand is transformed ONCE into one spectrum that every member's kernels read (member stride 0): n_batch + 1 input
 *     transforms per call instead of 2 n_batch.  Every member still writes its own four A' arrays per direction.  Scratch scales
 *     with max_batch (2 max_batch spectra, max_batch x the symmetric slabs and segment sums, max_batch second loss arrays);
 *     with max_batch <= 1 every allocation of the handle is what it was.
 *   - size-generic boxes: the batch runs member by member through the single calls; a shared operand is transformed again for
 *     every member there.
 *   - bfsm_collide_symmetric_batch is blocking and needs a handle that owns all directions; the _async forms are allocation-free
 *     after bfsm_create, graph-capturable after one evaluation outside a capture and tracked by bfsm_synchronize.  With
 *     BFSM_FLAG_PROFILE the counters cover the sequence; the byte model (symmetric_batch_moved_bytes_per_eval in
 *     csrc/bfsm_calls.hpp) scales with n_batch except for the transform of a shared operand.
 */
enum { BFSM_SHARE_NONE = 0, BFSM_SHARE_G = 1, BFSM_SHARE_F = 2 };
int bfsm_collide_symmetric_batch(bfsm_handle h, double* Q_dev, const double* g_dev, const double* f_dev, int n_batch, int share);
int bfsm_collide_symmetric_batch_partial_async(bfsm_handle h, double* Q_dev, const double* g_dev, const double* f_dev, int n_batch,
                                               int share, int with_loss, void* stream);
int bfsm_collide_bilinear_batch_partial_async(bfsm_handle h, double* Q_dev, const double* g_dev, const double* f_dev, int n_batch,
                                              int share, int with_loss, void* stream);

/*
 * Gain / loss split (new functionality; the presence of these symbols is the capability check, BFSM_VERSION stays 2).
 * Every entry point above returns the combined Q = Q+ - f nu[f]; these return its two terms apart:
 *     Qgain = Re IFFT(this handle's (partial) Q_gain_hat)   -- exactly what the combined call writes with with_loss = 0
 *     nu    = Re IFFT(beta2 f_hat / G)                       -- the collision frequency nu[f]; written only if with_loss != 0
 * so that Q = Qgain - f * nu (bilinear form: Q(g,f) = Qgain - g * nu, nu = nu[f]).  What an implicit or penalized time
 * integrator needs: the loss step f <- (f + dt Qgain) / (1 + dt nu), a bound mu >= max nu, the diagonal -nu[f] of L_f, the
 * time-step bound dt max nu.  Same kernels and bytes as the combined call; only the last tail kernel
 * differs (two real arrays written instead of f read and one written).
 *   - Qgain, nu, f (and g): device pointers to doubles, also on BFSM_F32 handles; batches are [n_batch][G] in all three
 *     arrays, 1 <= n_batch <= max_batch, and member i is bitwise the single call on member i ON THE SAME HANDLE.
 *   - with_loss = 0: nu may be NULL and is not touched.  On direction shards the caller sums Qgain over the ranks and
 *     exactly one rank passes with_loss != 0 (nu does not depend on the shard).
 *   - Qgain and nu must not overlap each other, f or g (BFSM_ERR_INVALID).
 *   - bfsm_collide_split and bfsm_collide_split_async (the forms without _partial) need a handle that owns ALL directions.
 *   - split is independent of the gain mode: faithful, BFSM_FLAG_EXACT_REDUCTIONS and BFSM_FLAG_HERMITIAN handles serve
 *     Q(f,f); the bilinear split on an exact-reduction handle returns BFSM_ERR_UNSUPPORTED and leaves the outputs untouched,
 *     like bfsm_collide_bilinear*.
 *   - N = 16 handles evaluate split calls on the plane-tile pipeline (as with BFSM_FLAG_NO_SMALL_PATH).
 *   - BFSM_FLAG_CONSERVE has NO effect on the split outputs: the projection P applies to Q, not to its two parts.  A caller
 *     who wants PQ assembles Q = Qgain - f * nu and calls bfsm_conserve_async on it.
 *   - bfsm_loss_rate_async computes nu alone, without any gain work (F1, beta2, one inverse transform), for n_batch
 *     distributions on any handle, a direction shard included; nu must not overlap f.
 *   - the _async forms are allocation-free after the first evaluation, graph-capturable and tracked by bfsm_synchronize like
 *     the other _async entry points; bfsm_collide_split is blocking.
 */
int bfsm_collide_split(bfsm_handle h, double* Qgain_dev, double* nu_dev, const double* f_dev);
int bfsm_collide_split_async(bfsm_handle h, double* Qgain_dev, double* nu_dev, const double* f_dev, void* stream);
int bfsm_collide_split_batch_partial_async(bfsm_handle h, double* Qgain_dev, double* nu_dev, const double* f_dev, int n_batch,
                                           int with_loss, void* stream);
int bfsm_collide_bilinear_split_partial_async(bfsm_handle h, double* Qgain_dev, double* nu_dev, const double* g_dev,
                                              const double* f_dev, int with_loss, void* stream);
int bfsm_loss_rate_async(bfsm_handle h, double* nu_dev, const double* f_dev, int n_batch, void* stream);

/* Q := PQ in place (the projection of BFSM_FLAG_CONSERVE, by the same kernels: bitwise the same result) for n_batch
 * consecutive arrays of G doubles, 1 <= n_batch <= max_batch, on any handle with or without the flag; enqueued on `stream`
 * like the other _async entry points (allocation-free, graph-capturable).  Null or misaligned Q, bad n_batch:
 * BFSM_ERR_INVALID. */
int bfsm_conserve_async(bfsm_handle h, double* Q_dev, int n_batch, void* stream);

/*
 * Macroscopic state of f and its Maxwellian on the device (new functionality; the presence of these symbols is the capability
 * check, BFSM_VERSION stays 2).  With dV = dx dy dz, d_a = 2L / n_a, and the grid v_a(i) = -L + (i + 1/2) d_a, a row of
 * BFSM_MOM_COUNT doubles per distribution:
 *     rho = dV sum f,   m = dV sum v f,   E = dV sum |v|^2 f  (= rho (|u|^2 + 3T)),   u = m / rho,   T = (E / rho - |u|^2) / 3,
 *     H = dV sum_{f > 0} f log f    (points with f <= 0 contribute 0);        rho == 0 gives u = T = 0.
 * bfsm_moments_async writes mom_dev[n_batch][BFSM_MOM_COUNT] from f_dev[n_batch][G]; f is not written.
 * bfsm_maxwellian_async writes M_dev[n_batch][G], M = rho (2 pi T)^(-3/2) exp(-|v - u|^2 / 2T), from rows in DEVICE memory, so
 * moments -> maxwellian needs no host round trip (what a BGK / ES-BGK closure or a penalized step reads, INTEGRATION.md
 * section 8).  A caller may fill the rows itself: only BFSM_MOM_RHO, BFSM_MOM_UX..UZ and BFSM_MOM_T are read.  A member whose
 * rho or T is not finite and positive (an empty or sign-indefinite f) gets M = 0 everywhere: the device cannot report an
 * error, and the other members of the batch are unaffected.
 *   - any handle: fused cube, size-generic box, N = 16, BFSM_F32 (the sums are fp64 whatever the transform precision), a
 *     direction shard, any flags; the results do not depend on any of these.
 *   - 1 <= n_batch <= max_batch; member i is bitwise the single call on member i on the same handle; repeated calls are
 *     bitwise identical (fixed-order sums, no atomics; the workgroup count depends on G only).
 *   - f_dev and M_dev must be 16-byte aligned.  BFSM_ERR_INVALID, with a message and nothing written: a null or misaligned
 *     pointer, a bad n_batch, mom overlapping f, M overlapping mom.
 *   - allocation-free after bfsm_create, graph-capturable and tracked by bfsm_synchronize like the other _async entry points.
 */
enum { BFSM_MOM_RHO = 0, BFSM_MOM_MX = 1, BFSM_MOM_MY = 2, BFSM_MOM_MZ = 3, BFSM_MOM_E = 4, BFSM_MOM_UX = 5, BFSM_MOM_UY = 6,
       BFSM_MOM_UZ = 7, BFSM_MOM_T = 8, BFSM_MOM_H = 9, BFSM_MOM_COUNT = 10 };
int bfsm_moments_async(bfsm_handle h, double* mom_dev, const double* f_dev, int n_batch, void* stream);
int bfsm_maxwellian_async(bfsm_handle h, double* M_dev, const double* mom_dev, int n_batch, void* stream);

/* Blocks until everything enqueued by this handle has completed: the work of every stream that was passed to one of
 * its entry points since the previous bfsm_synchronize is waited for (through events the handle recorded itself), not
 * only the most recent one; every distinct stream is tracked, however many.  The list is cleared whether or not the
 * wait succeeds, so a failure does not affect later calls. */
int bfsm_synchronize(bfsm_handle h);

/* Batched 3-D complex transform with the library's own kernels (counterpart of the cufftPlanMany plan,
 * CUDABoltzmannOperator.cu:88-100; used by the FFT unit tests that mirror cufft_benchmark.cu:150-207).
 * data_dev: batch * G interleaved complex of the handle's precision, transformed in place, unnormalised.
 * sign -1 = forward: physical [x][y][z] in, spectral-transposed [lx][lz][ly] out (the fused pipeline's spectral layout);
 * sign +1 = backward: [lx][lz][ly] in, [x][y][z] out.  1 <= batch <= 65535 (one grid dimension).
 * On boxes served by the size-generic path the spectral side is the natural [lx][ly][lz]. */
int bfsm_fft3d(bfsm_handle h, void* data_dev, int batch, int sign);

int bfsm_get_counters(bfsm_handle h, bfsm_counters* out);

/* == ~BoltzmannOperator() (CUDABoltzmannOperator.cu:224-261) */
int bfsm_destroy(bfsm_handle h);

/* Message of the last failure on this handle (or of the last failed bfsm_create when h == NULL). */
const char* bfsm_last_error(bfsm_handle h);

/* "HIP" -- what getBackendName() returns (CUDABoltzmannOperator.hpp:60-62 returns "CUDA"). */
const char* bfsm_backend_name(void);
int bfsm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BFSM_H */
