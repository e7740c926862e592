// bfsm_pipeline.hpp -- host-side plan (tables, direction chunks) and the launch sequence of one collision
// evaluation.  Pure C++17, no HIP types: the sequence is a template over a `Backend` that owns memory and
// launches the kernel bodies of bfsm_core.hpp.  bfsm_hip.hip provides the HIP backend (the product);
// tests/emu provides a host lock-step backend so the same plan + sequence is unit-tested without a GPU.
//
// What is computed ("the algorithm in one block"; Collisions/FFTWBoltzmannOperator.cpp:147-334):
//   f_hat = FFT(f)
//   for every direction b=(r,s) of this shard:   A1 = IFFT(e^{+i theta} f_hat / G), A2 = IFFT(e^{-i theta} f_hat / G)
//                                                 P_hat = FFT(A1 * A2)
//                                                 Q_hat += (1/G) w_r w_s rho_r^(gamma+2) * beta1(r,|l|) * P_hat
//   Q = Re IFFT(Q_hat) - Re(IFFT(beta2 f_hat / G)) * f
#pragma once
#include <cmath>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/bfsm.h"
#include "bfsm_core.hpp"

namespace bfsm {

struct Chunk {
    long long dir0;   // first direction, LOCAL index inside the shard (tables are shard-local)
    int n;            // directions in the chunk (may span several radial nodes)
    int per_group;    // directions per workgroup column of KA
    int seg0;         // first accumulation segment (== first slab) of the chunk
    int n_seg;        // segments of the chunk (grid.y of KC)
};

struct PlanInfo {
    int N = 0;
    int precision = 64;
    int n_gl = 0, n_sph = 0;
    // Work units are EFFECTIVE directions e = r*sph_eff + s.  Reference-faithful mode: sph_eff = n_sph, weight_mult = 1
    // (one unit per quadrature direction).  Exact-reduction mode on an antipodal design: sph_eff = n_sph/2,
    // weight_mult = 2 (direction s and its antipode s + n_sph/2 give the identical product A1*A2).
    int sph_eff = 0;
    int weight_mult = 1;
    bool exact_reductions = false;         // BFSM_FLAG_EXACT_REDUCTIONS
    bool hermitian = false;                // BFSM_FLAG_HERMITIAN: store only the planes lx = 0..N/2 of A1', A2' 
    bool antipodal = false;                // design satisfies sigma_{s+M/2} == -sigma_s and w equal, bit-exactly
    long long full_begin = 0, full_end = 0;  // the shard as given, in full quadrature directions b = r*n_sph + s
    long long dir_begin = 0, dir_end = 0;  // the shard in effective directions
    int max_chunk = 1024;
    int groups = 8;                        // target workgroup columns per x-plane (>= 2 workgroups per CU)
    std::vector<Segment> segs;             // accumulation segments of all chunks, in slab order
    int n2stride = 0;                      // 3*(N/2)^2 + 1
    std::vector<Chunk> chunks;
    int largest_chunk = 0;
    size_t Gtot = 0;                       // grid points when the plan is not a cube of N (size-generic path, N = 0)
    bool gen_plane = false;                // size-generic path: y and z pass fused through LDS (12 instead of 18 array moves)
    bool gen_fused = false;                // size-generic path: plane / x-line / plane-accumulate kernels (6 array moves)
    int gen_slabs = 0;                     // ... and the partial-sum slabs its chunks write
    int gen_moves = 18;                    // size-generic path: array moves per direction of the sequence chosen (6 ... 18)
    size_t G() const { return Gtot ? Gtot : (size_t)N * N * N; }
    long long n_dirs() const { return dir_end - dir_begin; }
};

// sincc(x) = sin(x+eps)/(x+eps)  (Collisions/FFTWBoltzmannOperator.hpp:17-21, BoltzmannCUDAKernels.hpp:17-29)
inline double sincc_ref(double x) {
    const double eps = DBL_EPSILON;
    return std::sin(x + eps) / (x + eps);
}

// Cubic grids of these sizes (N = Q T^2 with T = 4 or 8 threads per line) run on the fused three-kernel pipeline; every
// other supported grid on the size-generic path of bfsm_generic.hpp.
inline bool fused_grid(const bfsm_desc& d) {
    const int N = d.nvx;
    return d.nvx == d.nvy && d.nvx == d.nvz && (N == 16 || N == 24 || N == 32 || N == 40 || N == 48 || N == 64 || N == 80 || N == 96 || N == 128);
}

// An axis length the library has a transform for: even (the reference's mode tables need it,
// FFTWBoltzmannOperator.cpp:50-57), 4 <= n <= 256, prime factors 2, 3, 5, 7, 11, 13.
inline bool axis_supported(int n) {
    if (n < 4 || n > 256 || n % 2 != 0) return false;
    for (int p : {2, 3, 5, 7, 11, 13}) while (n % p == 0) n /= p;
    return n == 1;
}

inline int validate_desc(const bfsm_desc& d, std::string& err) {
    if (!axis_supported(d.nvx) || !axis_supported(d.nvy) || !axis_supported(d.nvz)) {
        err = "every grid extent must be even, in [4, 256], with prime factors 2, 3, 5, 7, 11, 13 only";
        return BFSM_ERR_UNSUPPORTED;
    }
    if (d.precision != BFSM_F64 && d.precision != BFSM_F32) { err = "precision must be BFSM_F64 or BFSM_F32"; return BFSM_ERR_INVALID; }
    if (d.n_gl < 1 || d.n_sph < 1) { err = "n_gl and n_sph must be positive"; return BFSM_ERR_INVALID; }
    if (!d.gl_nodes || !d.gl_wts || !d.sph_wts || !d.sx || !d.sy || !d.sz) { err = "null quadrature array"; return BFSM_ERR_INVALID; }
    if (!(d.L > 0)) { err = "L must be positive"; return BFSM_ERR_INVALID; }
    const long long B = (long long)d.n_gl * d.n_sph;
    if (!(d.dir_begin == 0 && d.dir_end == 0) && (d.dir_begin < 0 || d.dir_end > B || d.dir_begin > d.dir_end)) {
        err = "direction shard out of range"; return BFSM_ERR_INVALID;
    }
    if (d.max_chunk < 0 || d.max_chunk > 16384) { err = "max_chunk must be in [0, 16384] (it is a grid dimension)"; return BFSM_ERR_INVALID; }
    if (d.max_batch < 0 || d.max_batch > 65535) { err = "max_batch must be in [0, 65535]"; return BFSM_ERR_INVALID; }
    if (!fused_grid(d) && d.max_chunk > 16383) { err = "max_chunk too large for this grid"; return BFSM_ERR_INVALID; }
    if ((d.flags & BFSM_FLAG_HERMITIAN) && !(d.flags & BFSM_FLAG_EXACT_REDUCTIONS)) {
        err = "BFSM_FLAG_HERMITIAN is an additional exact reduction: set BFSM_FLAG_EXACT_REDUCTIONS as well";
        return BFSM_ERR_INVALID;
    }
    return BFSM_OK;
}

// Workgroups a plane-parallel kernel (KA, KC) should offer: two 512-thread workgroups per CU at N >= 64 (what the
// 65 KiB tiles allow); the small grids have 128- and 64-thread workgroups, so the same 16 waves per CU take 8 / 16
// workgroups per CU.
// A handle created for batches of nb distributions multiplies every grid by nb, so the per-distribution target shrinks
// accordingly (never below 512: fewer, longer segments mean fewer slabs to write and reduce).
inline int target_workgroups(int N, int max_batch = 1) {
    const int single = N >= 64 ? 512 : (N == 32 ? 2048 : 1024);
    const int nb = max_batch > 1 ? max_batch : 1;
    return single / nb > 512 ? single / nb : 512;
}

// The shard of a handle in full quadrature directions b = r * n_sph + s: [dir_begin, dir_end), or all of them (0, 0)
inline void shard_range(const bfsm_desc& d, long long& begin, long long& end) {
    const long long B = (long long)d.n_gl * d.n_sph;
    if (d.dir_begin == 0 && d.dir_end == 0) { begin = 0; end = B; }
    else { begin = d.dir_begin; end = d.dir_end; }
}

inline PlanInfo make_plan(const bfsm_desc& d) {
    PlanInfo p;
    p.N = d.nvx;
    p.precision = d.precision;
    p.n_gl = d.n_gl;
    p.n_sph = d.n_sph;
    shard_range(d, p.full_begin, p.full_end);
    p.exact_reductions = (d.flags & BFSM_FLAG_EXACT_REDUCTIONS) != 0;
    p.hermitian = p.exact_reductions && (d.flags & BFSM_FLAG_HERMITIAN) != 0;
    p.sph_eff = d.n_sph;
    if (p.exact_reductions && d.n_sph % 2 == 0) {
        const int h = d.n_sph / 2;
        bool anti = true;
        for (int s = 0; s < h && anti; ++s)
            anti = d.sx[s + h] == -d.sx[s] && d.sy[s + h] == -d.sy[s] && d.sz[s + h] == -d.sz[s] &&
                   d.sph_wts[s + h] == d.sph_wts[s];
        if (anti) { p.antipodal = true; p.sph_eff = h; p.weight_mult = 2; }
    }
    // a shard of full directions maps to the proportional range of effective directions (monotone, so the ranks'
    // ranges still tile the whole set exactly once)
    p.dir_begin = p.full_begin * p.sph_eff / d.n_sph;
    p.dir_end = p.full_end * p.sph_eff / d.n_sph;
    // Directions resident at once.  Sized for 288 GB of HBM: by default the whole shard (up to 1024 directions,
    // i.e. 8 GiB of A1'/A2' scratch at N=64 fp64) is one chunk, so an evaluation is ~8 launches.
    p.max_chunk = d.max_chunk > 0 ? d.max_chunk : 1024;
    p.groups = (target_workgroups(p.N, d.max_batch) + p.N - 1) / p.N;
    // KC only streams and sums until its one transform per segment, so at N = 32 half as many, twice as long segments
    // win: half the slabs to write and reduce (config 2: KC 42 -> 40 us, reduce 12 -> 8 us)
    if (p.N == 32) p.groups /= 2;
    if (p.groups < 1) p.groups = 1;
    p.n2stride = 3 * (p.N / 2) * (p.N / 2) + 1;
    const long long len = p.dir_end - p.dir_begin;
    if (len > 0) {
        const long long pieces = (len + p.max_chunk - 1) / p.max_chunk;
        const long long piece = (len + pieces - 1) / pieces;
        for (long long o = 0; o < len; o += piece) {
            Chunk c;
            c.dir0 = o;
            c.n = (int)((o + piece <= len) ? piece : (len - o));
            c.per_group = (c.n + p.groups - 1) / p.groups;
            c.seg0 = (int)p.segs.size();
            // radial runs inside the chunk; every run is cut into `cuts` near-equal segments so that the chunk
            // offers at least `groups` accumulating workgroups per x-plane
            const long long g0 = p.dir_begin + o, g1 = g0 + c.n;
            const int r_first = (int)(g0 / p.sph_eff), r_last = (int)((g1 - 1) / p.sph_eff);
            const int runs = r_last - r_first + 1;
            int cuts = (p.groups + runs - 1) / runs;
            // KC runs N x segments workgroups; with the large tiles only `resident` of them fit the GPU at once
            // (one per CU at N = 128, two at N = 64), so a segment count that is not a multiple of resident / N leaves
            // a partly empty last round (config 5: 5 runs -> 640 workgroups = 2.5 rounds; 10 segments = 5 full rounds)
            const int resident = p.N >= 128 ? 256 : (p.N == 64 ? 512 : 0);
            if (resident > 0 && resident % p.N == 0) {
                const int unit = resident / p.N;
                for (int extra = 0; extra < unit && (runs * cuts) % unit != 0; ++extra) ++cuts;
            } else if (p.N == 48 || p.N == 96 || p.N == 80 || p.N == 24 || p.N == 40) {
                // sizes whose row count does not divide the resident set: among cuts .. cuts + 3 take the count that
                // fills its rounds of resident workgroups best (N = 96 / 80: one / two or three workgroups per CU by LDS;
                // N = 48: four / eight; N = 24: one-wave workgroups, 16 per CU)
                const bool f64 = p.precision == BFSM_F64;
                const int res = p.N == 96 ? (f64 ? 256 : 512) : p.N == 80 ? (f64 ? 256 : 768) : p.N == 48 ? (f64 ? 1024 : 2048) : (p.N == 40 ? 2048 : 4096);
                int best = cuts;
                double best_u = 0;
                for (int c2 = cuts; c2 <= cuts + 3; ++c2) {
                    const long long w = (long long)p.N * runs * c2, rounds = (w + res - 1) / res;
                    const double u = (double)w / (double)(rounds * res);
                    if (u > best_u + 0.02) { best_u = u; best = c2; }
                }
                cuts = best;
            }
            for (int r = r_first; r <= r_last; ++r) {
                long long a0 = (long long)r * p.sph_eff, a1 = a0 + p.sph_eff;
                if (a0 < g0) a0 = g0;
                if (a1 > g1) a1 = g1;
                const long long rl = a1 - a0;
                const long long k = rl < cuts ? rl : cuts;
                for (long long j = 0; j < k; ++j) {
                    const long long s0 = a0 + rl * j / k, s1 = a0 + rl * (j + 1) / k;
                    Segment sg;
                    sg.d0 = (int)(s0 - g0);
                    sg.n = (int)(s1 - s0);
                    sg.r = r;
                    sg.pad = 0;
                    p.segs.push_back(sg);
                }
            }
            c.n_seg = (int)p.segs.size() - c.seg0;
            if (c.n > p.largest_chunk) p.largest_chunk = c.n;
            p.chunks.push_back(c);
        }
    }
    return p;
}

// Host tables, built in double / long double, then narrowed to T.
template <typename T>
struct HostTables {
    std::vector<cx<T>> tw;                 // [N]
    std::vector<cx<T>> phx, phy, phz;      // [n_dirs][N]
    std::vector<T> dirw;                   // [n_dirs]
    std::vector<T> beta1;                  // [n_gl][n2stride]
    std::vector<T> beta2;                  // [n2stride]
};

// The pieces of the host tables, shared by build_tables() and GenericPipeline::init: one copy of the reference's formulas
constexpr double TABLE_PI = 3.14159265358979323846;  // Utilities/constants.hpp:7
constexpr long double TABLE_PI_L = 3.141592653589793238462643383279502884L;
// exp(-2 pi i k / n), k < n
template <typename T>
std::vector<cx<T>> twiddle_table(int n) {
    std::vector<cx<T>> tw(n);
    for (int k = 0; k < n; ++k) {
        const long double a = -2.0L * TABLE_PI_L * (long double)k / (long double)n;
        tw[k] = {(T)cosl(a), (T)sinl(a)};
    }
    return tw;
}
// theta(l) = -(pi/(2L)) rho_r (l . sigma_s)   (FFTWBoltzmannOperator.cpp:205-209) is separable in lx, ly, lz: the factor k of
// radial node r, and one direction's row exp(i k l sigma) along an axis of n points, l the FFT-order mode (cpp:50-57).
// scale: a factor applied in double; null: the value narrows straight to T.
inline long double phase_k(const bfsm_desc& d, int r) {
    return -((long double)TABLE_PI / (2.0L * (long double)d.L)) * (long double)d.gl_nodes[r];
}
template <typename T>
void phase_row(cx<T>* dst, int n, long double k, double sigma, const double* scale) {
    for (int j = 0; j < n; ++j) {
        const int l = j < n / 2 ? j : j - n;
        const long double a = k * (long double)l * (long double)sigma;
        if (scale) dst[j] = {(T)(*scale * (double)cosl(a)), (T)(*scale * (double)sinl(a))};
        else dst[j] = {(T)cosl(a), (T)sinl(a)};
    }
}
// weight = fft_scale * gl_wts[r] * spherical_wts[s] * pow(gl_nodes[r], gamma + 2)   (cpp:252)
inline double direction_weight(const bfsm_desc& d, int r, int s, double fft_scale) {
    return fft_scale * d.gl_wts[r] * d.sph_wts[s] * std::pow(d.gl_nodes[r], d.gamma + 2);
}
// beta1 [n_gl][n2stride] and beta2 [n2stride] over |l|^2 = n2
template <typename T>
void beta_tables(const bfsm_desc& d, int n2stride, double fft_scale, std::vector<T>& beta1, std::vector<T>& beta2) {
    const double pi = TABLE_PI;
    beta1.resize((size_t)d.n_gl * n2stride);
    beta2.resize((size_t)n2stride);
    for (int n2 = 0; n2 < n2stride; ++n2) {
        const double norm_l = std::sqrt((double)n2);
        double b2 = 0;
        for (int r = 0; r < d.n_gl; ++r) {
            // beta1 = 4 pi b_gamma sincc(pi rho_r |l| / (2L))   (cpp:261-262)
            beta1[(size_t)r * n2stride + n2] = (T)(4 * pi * d.b_gamma * sincc_ref(pi * d.gl_nodes[r] * norm_l / (2 * d.L)));
            // beta2 += 16 pi^2 b_gamma w_r rho_r^(gamma+2) sincc(pi rho_r |l| / L)   (cpp:290-293)
            b2 += 16 * pi * pi * d.b_gamma * d.gl_wts[r] * std::pow(d.gl_nodes[r], d.gamma + 2) *
                  sincc_ref(pi * d.gl_nodes[r] * norm_l / d.L);
        }
        beta2[n2] = (T)(fft_scale * b2);   // cpp:295-296 folds fft_scale
    }
}

template <typename T>
HostTables<T> build_tables(const bfsm_desc& d, const PlanInfo& p) {
    HostTables<T> t;
    const int N = p.N;
    const double fft_scale = 1.0 / (double)p.G();   // FFTWBoltzmannOperator.cpp:162
    t.tw = twiddle_table<T>(N);
    const long long nd = p.n_dirs();
    t.phx.resize((size_t)nd * N); t.phy.resize((size_t)nd * N); t.phz.resize((size_t)nd * N);
    t.dirw.resize((size_t)nd);
    for (long long i = 0; i < nd; ++i) {
        const long long b = p.dir_begin + i;
        const int r = (int)(b / p.sph_eff), s = (int)(b % p.sph_eff);   // s < n_sph/2 when antipodal pairs are merged
        const long double k = phase_k(d, r);
        phase_row(&t.phx[(size_t)i * N], N, k, d.sx[s], &fft_scale);
        phase_row(&t.phy[(size_t)i * N], N, k, d.sy[s], nullptr);
        phase_row(&t.phz[(size_t)i * N], N, k, d.sz[s], nullptr);
        t.dirw[(size_t)i] = (T)(p.weight_mult * (direction_weight(d, r, s, fft_scale)));
    }
    beta_tables(d, p.n2stride, fft_scale, t.beta1, t.beta2);
    return t;
}

// Kernels of the N = 16 whole-direction path (bfsm_core.hpp, "small_*").
enum class SK { Gain, Reduce };

// Kernel identifiers the backend dispatches on.
enum class K { TileFwdReal, LineFwd, LineInv, TileFwd, TileInv, GainInv, GainLine, GainFwd, Reduce, TailInv, TailLine, GainLineAcc,
               NyqRows, GainLineAccH, GainInvNyq,     // appended: the numeric values of the others appear in profiles
               GainInvTwo };                          // KA storing two arrays on a geometry whose default is interleaved pairs

// 1-D (x-axis) kernels take Wg<N>::NPL columns per workgroup, 2-D tile kernels a whole N x N tile.
constexpr bool is_line_kind(K k) {
    return k == K::LineFwd || k == K::LineInv || k == K::GainLine || k == K::GainLineAcc || k == K::TailLine ||
           k == K::NyqRows || k == K::GainLineAccH;
}

// Threads and dynamic LDS bytes of a launch of kernel `kind`
template <K kind, int N>
constexpr int kernel_threads() {
    if (kind == K::GainInv && pair_tile<N>()) return pair_threads<N>();      // two tiles side by side (N = 32)
    return kind == K::Reduce ? 256 : (is_line_kind(kind) ? Wg<N>::LINE_THREADS : Wg<N>::THREADS);
}
template <K kind, int N, typename T>
constexpr size_t kernel_lds_bytes() {
    if (kind == K::GainInv && pair_tile<N>()) return pair_lds_bytes<N, T>();
    if (kind == K::GainInv && ka_xlane<N, T>()) return ka_xlane_lds_bytes<N, T>();
    if (kind == K::GainFwd) return kc_lds_bytes<N, T>();
    if (kind == K::GainInvNyq) return gain_inv_lds_bytes<N, T>();
    return kind == K::Reduce ? 0 : (is_line_kind(kind) ? line_lds_bytes<N, T>() : tile_lds_bytes<N, T>());
}
template <SK kind, typename T>
constexpr size_t small_kernel_lds_bytes() { return kind == SK::Reduce ? 256 * sizeof(double) : small_lds_bytes<T>(); }

// The body of kernel `kind` on one workgroup (prm: its parameters, ctx: the execution context): the one table from kernel
// identifiers to the bodies of bfsm_core.hpp, expanded inside namespace bfsm by the __global__ wrappers of bfsm_hip.hip and
// by the emulator's backend.  A macro, not a function: one more inlined frame between a __global__ wrapper and the body
// reorders the wrapper's stack slots, the optimiser then takes another path through several kernels, and the asm("+s")
// operands of DevCtx no longer all stay in SGPRs (K::GainInv, N = 48, fp64, bilinear stops compiling).
#define BFSM_RUN_BODY(kind, N, T, prm, ctx)                                                                                  \
    if constexpr (kind == K::TileFwdReal) body_tile_fwd_real<N, T>(prm, ctx);                                                \
    else if constexpr (kind == K::LineFwd) body_line<N, -1, T>(prm, ctx);                                                    \
    else if constexpr (kind == K::LineInv) body_line<N, +1, T>(prm, ctx);                                                    \
    else if constexpr (kind == K::TileFwd) body_tile_c2c<N, -1, T>(prm, ctx);                                                \
    else if constexpr (kind == K::TileInv) body_tile_c2c<N, +1, T>(prm, ctx);                                                \
    else if constexpr (kind == K::GainInv && pair_tile<N>()) body_gain_inv_pair<N, T>(prm, ctx);                             \
    else if constexpr (kind == K::GainInv) body_gain_inv<N, T>(prm, ctx);                                                    \
    else if constexpr (kind == K::GainLine) body_gain_line<N, T>(prm, ctx);                                                  \
    else if constexpr (kind == K::GainFwd) body_gain_fwd<N, T>(prm, ctx);                                                    \
    else if constexpr (kind == K::Reduce) body_reduce<N, T>(prm, ctx);                                                       \
    else if constexpr (kind == K::TailInv) body_tail_inv<N, T>(prm, ctx);                                                    \
    else if constexpr (kind == K::TailLine) body_tail_line<N, T>(prm, ctx);                                                  \
    else if constexpr (kind == K::GainLineAcc) body_gain_line_acc<N, T>(prm, ctx);                                           \
    else if constexpr (kind == K::NyqRows) body_nyq_rows<N, T>(prm, ctx);                                                    \
    else if constexpr (kind == K::GainLineAccH) body_gain_line_acc_h<N, T>(prm, ctx);                                        \
    else if constexpr (kind == K::GainInvNyq) {          /* only launched where nyq_rides_along<N>() */                      \
        if constexpr (nyq_rides_along<N>()) body_gain_inv_nyq<N, T>(prm, ctx);                                               \
    } else if constexpr (kind == K::GainInvTwo) {          /* only launched on ab_interleaved geometries (Hermitian mode) */ \
        if constexpr (ab_interleaved<N, T>()) body_gain_inv<N, T, false>(prm, ctx);                                          \
    }
#define BFSM_RUN_SMALL_BODY(kind, T, prm, ctx)                             \
    if constexpr (kind == SK::Gain) body_small_gain<T>(prm, ctx);          \
    else if constexpr (kind == SK::Reduce) body_small_reduce<T>(prm, ctx);

// fn(std::integral_constant<int, N>{}) for the cube size N of the fused pipeline (fused_grid); false: not one of them
// BFSM_FUSED_N_MAX (test harness builds only, e.g. a sanitizer build of the host emulator): larger cubes are not instantiated
#ifndef BFSM_FUSED_N_MAX
#define BFSM_FUSED_N_MAX 128
#endif
template <class F>
bool for_fused_n(int N, F&& fn) {
    if (N > BFSM_FUSED_N_MAX) return false;
    switch (N) {
        case 16: fn(std::integral_constant<int, 16>{}); return true;
        case 24: fn(std::integral_constant<int, 24>{}); return true;
#if BFSM_FUSED_N_MAX >= 128
        case 32: fn(std::integral_constant<int, 32>{}); return true;
        case 40: fn(std::integral_constant<int, 40>{}); return true;
        case 48: fn(std::integral_constant<int, 48>{}); return true;
        case 80: fn(std::integral_constant<int, 80>{}); return true;     // (80 before 64: the order the kernels have in the
        case 64: fn(std::integral_constant<int, 64>{}); return true;     // code object, which follows the instantiations here)
        case 96: fn(std::integral_constant<int, 96>{}); return true;
        case 128: fn(std::integral_constant<int, 128>{}); return true;
#endif
        default: return false;
    }
}

// The device allocations of one handle (Pipeline, GenericPipeline): every buffer is made here, so release_owned() frees
// exactly what init made.
template <class Backend>
struct DeviceBuffers {
    Backend* be = nullptr;
    std::vector<void*> owned;     // every device allocation of this handle
    template <typename U>
    bool dev_alloc(U*& dst, size_t n) {
        dst = (U*)be->alloc(n * sizeof(U));
        if (dst) owned.push_back(dst);
        return dst != nullptr;
    }
    template <typename U>
    bool dev_copy(U*& dst, const std::vector<U>& src) {
        if (!dev_alloc(dst, src.empty() ? 1 : src.size())) return false;
        if (!src.empty()) be->upload(dst, src.data(), src.size() * sizeof(U));
        return true;
    }
    void release_owned() { for (void* p : owned) be->release(p); owned.clear(); }
};

// Device-resident state of one handle.  `Backend` supplies:
//   void* alloc(size_t), void release(void*), void upload(void* dst, const void* src, size_t), void zero(void*, size_t)
//   template <K kind, typename T, class P> void launch(int grid_x, int grid_y, int grid_z, const P& params, int N)
//   void mark(int kind, double alg_bytes)              -- accounting tag of the next launch (kind < 0: untracked)
template <typename T, class Backend>
struct Pipeline : DeviceBuffers<Backend> {
    using DeviceBuffers<Backend>::be; using DeviceBuffers<Backend>::dev_alloc; using DeviceBuffers<Backend>::dev_copy;
    PlanInfo plan;
    // device buffers
    cx<T>* fhat = nullptr;
    cx<T>* tg = nullptr;          // the tail's gain and loss arrays: one block [2][max_batch G], tl = tg + max_batch G
    cx<T>* tl = nullptr;
    cx<T>* qhat = nullptr;
    cx<T>* a1 = nullptr;
    cx<T>* a2 = nullptr;
    cx<T>* pp = nullptr;          // P' (per-direction route of the faithful mode only): a1 itself (KB works in place)
                                  // unless the scratch is interleaved (own buffer)
    cx<T>* slab = nullptr;
    cx<T>* tw = nullptr;
    cx<T>* phx = nullptr;
    cx<T>* phy = nullptr;
    cx<T>* phz = nullptr;
    T* dirw = nullptr;
    T* beta1 = nullptr;
    T* beta2 = nullptr;
    Segment* segs = nullptr;
    // segment sums formed by the x-line kernel (every mode but the per-direction route of the faithful mode)
    cx<T>* pseg = nullptr;        // [segment][x][y][z]
    Segment* segs_unit = nullptr; // one single-slot segment per pseg entry, same r
    T* ones = nullptr;
    cx<T>* slab_sym = nullptr;    // symmetric form: [max_batch][2 slab_count] slabs and segment sums, [max_batch] second loss arrays
    cx<T>* pseg_sym = nullptr;
    cx<T>* tl_sym = nullptr;
    cx<T>* rnyq = nullptr;        // Hermitian mode: Nyquist rows [slot][sign][kind][N/2-1][N]
    size_t slab_count = 0;
    // N = 16 whole-direction path: one partial Q_hat per workgroup
    T* small_part = nullptr;      // [small_wgs + 1][G] real partial results
    int small_wgs = 0, small_per = 0;

    // A1' / A2' interleaved per element in one array (bfsm_core.hpp, ab_interleaved)
    bool pair_geometry() const { return plan.N == 128 && ab_interleaved<128, T>(); }
    bool interleaved() const { return pair_geometry() && !plan.hermitian; }
    // the x-line kernel forms the segment sums (pseg) and ONE KC pass over them follows all chunks; false: the faithful
    // mode's per-direction route (KB writes every P'_d, one KC per chunk reads them back)
    bool segment_sums() const { return plan.exact_reductions || kb_sums_segments_n<T>(plan.N); }
    int a_planes = 0;        // lx planes of A1' / A2' kept per direction (N, or N/2 + 1 in the Hermitian mode)
    size_t r_per_dir() const { return (size_t)4 * (plan.N / 2 - 1) * plan.N; }
    int max_batch = 1;       // distributions evaluated per call; scratch scales with it
    size_t cap = 1;          // directions resident at once (largest chunk)

    int init(const bfsm_desc& d, Backend* backend, std::string& err) {
        be = backend;
        plan = make_plan(d);
        HostTables<T> t = build_tables<T>(d, plan);
        const size_t G = plan.G();
        cap = (size_t)(plan.largest_chunk > 0 ? plan.largest_chunk : 1);
        max_batch = d.max_batch > 1 ? d.max_batch : 1;
        const size_t nb = (size_t)max_batch;
        slab_count = plan.segs.size();
        const size_t nslab = slab_count ? slab_count : 1;
        bool ok = true;
        // two spectra per member: the bilinear and symmetric forms keep g_hat [max_batch][G] and f_hat [max_batch][G]
        // (collide_bilinear, collide_pairs); two in all on a max_batch <= 1 handle, as ever
        ok = ok && dev_alloc(fhat, 2 * nb * G);
        ok = ok && dev_alloc(tg, 2 * nb * G);
        if (ok) tl = tg + nb * G;
        ok = ok && dev_alloc(qhat, nb * G);
        a_planes = plan.hermitian ? plan.N / 2 + 1 : plan.N;
        const size_t Gp = (size_t)a_planes * plan.N * plan.N;       // elements of A1' / A2' per direction
        if (interleaved()) {
            // {A1', A2'} side by side in a1; a KB that writes every P'_d needs a buffer of its own for it (see ab_interleaved)
            ok = ok && dev_alloc(a1, 2 * nb * cap * Gp);
            if (!segment_sums()) ok = ok && dev_alloc(pp, nb * cap * G);
        } else {
            ok = ok && dev_alloc(a1, nb * cap * Gp);
            ok = ok && dev_alloc(a2, nb * cap * Gp);
            pp = a1;
        }
        if (plan.hermitian) ok = ok && dev_alloc(rnyq, nb * cap * r_per_dir());
        // the symmetric form Qs(g,f) runs two gain passes per chunk, the second into segment sums and slabs of its own: the
        // segment tables twice over (entry slab_count + i = entry i), and buffers of its own at the end of init
        std::vector<Segment> segs2(plan.segs);
        segs2.insert(segs2.end(), plan.segs.begin(), plan.segs.end());
        ok = ok && dev_alloc(slab, nb * nslab * G);
        ok = ok && dev_copy(tw, t.tw) && dev_copy(phx, t.phx) && dev_copy(phy, t.phy) && dev_copy(phz, t.phz);
        ok = ok && dev_copy(dirw, t.dirw) && dev_copy(beta1, t.beta1) && dev_copy(beta2, t.beta2) && dev_copy(segs, segs2);
        if (ok && segment_sums()) {
            std::vector<Segment> unit(segs2.size());
            for (size_t i = 0; i < unit.size(); ++i) unit[i] = Segment{(int)i, 1, segs2[i].r, 0};
            std::vector<T> one(unit.size() ? unit.size() : 1, (T)1);
            ok = ok && dev_alloc(pseg, nb * nslab * G);
            ok = ok && dev_copy(segs_unit, unit) && dev_copy(ones, one);
        }
        if (ok && plan.N == SMALL_N && !(d.flags & BFSM_FLAG_NO_SMALL_PATH) && plan.n_dirs() > 0 && max_batch == 1) {
            // a whole direction fits one workgroup: single evaluations take the three-launch path of collide_small
            // (handles created for batches keep one set of kernels: a single evaluation on them is bitwise a batch member)
            const long long nd = plan.n_dirs();
            const long long wg = nd < 256 ? nd : 256;
            small_per = (int)((nd + wg - 1) / wg);
            small_wgs = (int)((nd + small_per - 1) / small_per);
            ok = ok && dev_alloc(small_part, (size_t)(small_wgs + 1) * G);
        }
        // Scratch of the symmetric form alone, allocated last so that every buffer of the other entry points is made in the order
        // and size it always was: per member 2 x slab_count slabs and segment sums (member stride 2 x slab_count x G) and the
        // second loss array; on a max_batch <= 1 handle the sizes they always had
        ok = ok && dev_alloc(slab_sym, nb * 2 * nslab * G);
        if (segment_sums()) ok = ok && dev_alloc(pseg_sym, nb * 2 * nslab * G);
        ok = ok && dev_alloc(tl_sym, nb * G);
        if (!ok) { err = "device allocation failed"; return BFSM_ERR_NOMEM; }
        return BFSM_OK;
    }

    // Whole evaluation on the N = 16 path (two launches, see bfsm_core.hpp); Q = gain [- loss]
    bool small_path(int nb) const { return small_part != nullptr && nb == 1; }
    void collide_small(double* Q_dev, const double* f_dev, bool with_loss) {
        const double Gc = (double)plan.G() * cbytes();
        // the loss term: one more workgroup while the gain workgroups leave a CU free (one workgroup per CU: 136 KiB of
        // LDS), otherwise workgroup 0 carries it next to its own share
        const bool extra = with_loss && small_wgs < 256;
        SmallGainParams<T> kg{f_dev, small_part, beta2, with_loss ? (extra ? small_wgs : 0) : -1, small_wgs, phx, phy, phz, dirw,
                              beta1, plan.n2stride, (int)plan.n_dirs(), small_per, plan.dir_begin, plan.sph_eff,
                              plan.exact_reductions ? 1 : 0};
        const int n_part = small_wgs + (extra ? 1 : 0);
        be->mark(BFSM_K_GAIN_LINE, 0.5 * n_part * Gc);
        be->template launch_small<SK::Gain, T>(n_part, kg);
        SmallReduceParams<T> kr{small_part, Q_dev, n_part};
        be->mark(BFSM_K_REDUCE, 0.5 * (n_part + 1.0) * Gc);
        be->template launch_small<SK::Reduce, T>((int)(plan.G() / 16), kr);
    }

    void destroy() {
        if (!be) return;
        this->release_owned();
        *this = Pipeline();       // no pointer to released memory survives
    }

    double cbytes() const { return (double)sizeof(cx<T>); }
    int line_blocks() const { return plan.N * plan.N / line_npl(plan.N); }   // Wg<N>::NPL columns per workgroup
    static bool kn_rides_along(int n) { return n == 64 && nyq_rides_along<64>(); }

    // f_hat = FFT(f), then the gain term of this shard into qhat (partial Q_gain_hat, spectral layout).
    // nb distributions f_dev[nb][G] are processed by the same launches (grid.z / grid.y = batch member); all
    // per-distribution buffers are [nb][...].
    // Fusing the slab reduce into the first tail kernel saves a launch and a pass over Q_hat, but that kernel has only
    // N (x 2) workgroups, each walking all slabs: it pays for few slabs (a 1/8 shard of cfg3: 0.445 -> 0.439 ms per
    // evaluation) and loses against the wide reduce kernel for many (cfg2, 64 slabs: 4.0 k -> 2.8 k evaluations/s).
    bool fuse_reduce() const { return slab_count <= 8; }
    bool batch_together() const { return true; }          // batches of distributions share every launch

    // do_reduce = false leaves the slabs un-summed (qhat is not written): for callers that continue with
    // finish(..., from_slabs = true) in the same call and never expose qhat.
    void gain_partial(const double* f_dev, int nb = 1, bool do_reduce = true) {
        spectrum(f_dev, fhat, nb);
        gain_spectra(nb, do_reduce, nullptr);
    }

    // F1: out = FFT(f)  (CUDABoltzmannOperator.cu:133-140), spectral layout
    void spectrum(const double* f_dev, cx<T>* out, int nb) {
        const int N = plan.N;
        const double Gc = (double)plan.G() * cbytes() * nb;
        TileFwdRealParams<T> pa{f_dev, tg, tw};
        be->mark(BFSM_K_FFT_F, 1.5 * Gc);
        be->template launch<K::TileFwdReal, T>(N, nb, 1, pa, N);
        LineParams<T> pb{tg, out, tw};
        be->mark(BFSM_K_FFT_F, 2.0 * Gc);
        be->template launch<K::LineFwd, T>(line_blocks(), nb, 1, pb, N);
    }

    // Bilinear form Q(g,f) (include/bfsm.h, bfsm_collide_bilinear): A1' from g_hat, A2' from f_hat, loss = g * Re IFFT(beta2
    // f_hat / G).  One distribution; the faithful mode only (the exact reductions merge antipodes, which assumes g = f); N = 16
    // takes the plane-tile pipeline (the whole-direction kernels have no room for a second cube).  g_hat in fhat, f_hat in
    // fhat + G (init reserves two spectra).
    cx<T>* fhat_b() const { return fhat + plan.G(); }
    // nu_dev: the split form (finish)
    void collide_bilinear(double* Q_dev, const double* g_dev, const double* f_dev, bool with_loss, double* nu_dev = nullptr) {
        spectrum(g_dev, fhat, 1);
        if (f_dev == g_dev) {     // Q(f,f) through the bilinear kernels: one transform, both operands read the same spectrum
            const bool fu = fuse_reduce();
            gain_spectra(1, !fu, fhat);
            finish(Q_dev, g_dev, with_loss, 1, fu, fhat, nu_dev);
            return;
        }
        spectrum(f_dev, fhat_b(), 1);
        const bool fu = fuse_reduce();
        gain_spectra(1, !fu, fhat_b());
        finish(Q_dev, g_dev, with_loss, 1, fu, fhat_b(), nu_dev);
    }

    // Symmetric form Qs(g,f) = Q(g,f) + Q(f,g) (include/bfsm.h, bfsm_collide_symmetric*), every mode.  g_hat in fhat, f_hat in
    // fhat + G; per chunk two gain passes with the spectra exchanged (gain_spectra, symmetric); one KC, one reduce (fused into
    // the tail when the 2 x slab_count slabs are at most 8), one tail with both loss terms.  On a merged plan (exact
    // reductions, antipodal rule) the two passes per effective direction s < M/2 are P_s(g,f) and P_s(f,g) = P_{s+M/2}(g,f)
    // with the doubled weight: the whole symmetric gain from M/2 directions.  On every other plan they are the two gains.
    bool fuse_reduce_symmetric() const { return 2 * slab_count <= 8; }
    void collide_symmetric(double* Q_dev, const double* g_dev, const double* f_dev, bool with_loss) {
        spectrum(g_dev, fhat, 1);
        const cx<T>* fb = fhat;                                   // g == f: one transform, both operands read the same spectrum
        if (f_dev != g_dev) { spectrum(f_dev, fhat_b(), 1); fb = fhat_b(); }
        const bool fu = fuse_reduce_symmetric();
        gain_spectra(1, !fu, fb, true);
        const int N = plan.N;
        const double Gc = (double)plan.G() * cbytes();
        const size_t n_slabs = 2 * slab_count, s_bs = (slab_count ? slab_count : 1) * plan.G();
        // tail: gain plane, beta2 f_hat (multiplied by g), beta2 g_hat (multiplied by f)
        TailInvSymParams<T> ta{{qhat, fb, beta2, tg, (long long)(tl - tg), tw, slab_sym, beta1, segs, fu ? (int)n_slabs : -1, plan.n2stride, s_bs},
                               (long long)(fhat - fb), (long long)(tl_sym - tg)};
        be->mark(BFSM_K_TAIL, ((with_loss ? 6.0 : 2.0) + (fu ? (double)n_slabs - 1.0 : 0.0)) * Gc);
        be->template launch<K::TailInv, T>(N, with_loss ? 3 : 1, 1, ta, N);
        TailLineSymParams<T> tb{{tg, tl, g_dev, Q_dev, tw, with_loss ? 1 : 0}, tl_sym, f_dev};
        be->mark(BFSM_K_TAIL, (with_loss ? 5.0 : 1.5) * Gc);
        be->template launch<K::TailLine, T>(line_blocks(), 1, 1, tb, N);
    }

    // Batched two-operand forms (include/bfsm.h, bfsm_collide_symmetric_batch*, bfsm_collide_bilinear_batch*): member i of Q is
    // Qs(g_i, f_i) (symmetric) or Q(g_i, f_i) for nb <= max_batch members, every launch covering the batch.  share
    // (BFSM_SHARE_G / BFSM_SHARE_F): that operand is ONE array all members read -- transformed once into one spectrum, read by
    // the kernels with a member stride of 0.  g_hat at fhat [max_batch][G], f_hat behind it; with nb = 1 the launches of
    // collide_symmetric / collide_bilinear, and every member is bitwise what they give on that member's operands.
    static constexpr bool pair_batches = true;        // one sequence for the whole batch (GenericPipeline: member by member)
    void collide_pairs(double* Q_dev, const double* g_dev, const double* f_dev, int nb, int share, bool with_loss, bool symmetric) {
        const int N = plan.N;
        const size_t G = plan.G();
        const size_t g_bs = share == BFSM_SHARE_G ? 0 : G, f_bs = share == BFSM_SHARE_F ? 0 : G;
        cx<T>* const ghat = fhat;
        cx<T>* const fhat_f = fhat + (size_t)max_batch * G;
        spectrum(g_dev, ghat, g_bs ? nb : 1);
        const cx<T>* fb = ghat;                                   // g == f: one transform per member, both operands read it
        if (!(f_dev == g_dev && share == BFSM_SHARE_NONE)) { spectrum(f_dev, fhat_f, f_bs ? nb : 1); fb = fhat_f; }
        const OperandSpectra sp{ghat, fb, g_bs, f_bs};
        const double Gc = (double)G * cbytes() * nb;
        const size_t nslab = slab_count ? slab_count : 1;
        if (symmetric) {
            const bool fu = fuse_reduce_symmetric();
            gain_spectra(nb, !fu, nullptr, true, &sp);
            const size_t n_slabs = 2 * slab_count;
            TailInvSymBatchParams<T> ta{};
            static_cast<TailInvParams<T>&>(ta) = TailInvParams<T>{qhat, fb, beta2, tg, (long long)(tl - tg), tw, slab_sym, beta1, segs,
                                                                   fu ? (int)n_slabs : -1, plan.n2stride, 2 * nslab * G};
            ta.fhat2_off = (long long)(ghat - fb);
            ta.tl2_off = (long long)(tl_sym - tg);
            ta.f_bstride = f_bs;
            ta.f2_bstride = g_bs;
            be->mark(BFSM_K_TAIL, ((with_loss ? 6.0 : 2.0) + (fu ? (double)n_slabs - 1.0 : 0.0)) * Gc);
            be->template launch<K::TailInv, T>(N, with_loss ? 3 : 1, nb, ta, N);
            TailLineSymBatchParams<T> tb{};
            static_cast<TailLineParams<T>&>(tb) = TailLineParams<T>{tg, tl, g_dev, Q_dev, tw, with_loss ? 1 : 0};
            tb.tl2 = tl_sym;
            tb.f2 = f_dev;
            tb.f_bstride = g_bs;
            tb.f2_bstride = f_bs;
            be->mark(BFSM_K_TAIL, (with_loss ? 5.0 : 1.5) * Gc);
            be->template launch<K::TailLine, T>(line_blocks(), nb, 1, tb, N);
        } else {
            const bool fu = fuse_reduce();
            gain_spectra(nb, !fu, nullptr, false, &sp);
            TailInvBatchParams<T> ta{};
            static_cast<TailInvParams<T>&>(ta) = TailInvParams<T>{qhat, fb, beta2, tg, (long long)(tl - tg), tw, slab, beta1, segs,
                                                                   fu ? (int)slab_count : -1, plan.n2stride, nslab * G};
            ta.f_bstride = f_bs;
            be->mark(BFSM_K_TAIL, ((with_loss ? 4.0 : 2.0) + (fu ? (double)slab_count - 1.0 : 0.0)) * Gc);
            be->template launch<K::TailInv, T>(N, with_loss ? 2 : 1, nb, ta, N);
            TailLineBatchParams<T> tb{};
            static_cast<TailLineParams<T>&>(tb) = TailLineParams<T>{tg, tl, g_dev, Q_dev, tw, with_loss ? 1 : 0};
            tb.f_bstride = g_bs;
            be->mark(BFSM_K_TAIL, (with_loss ? 3.0 : 1.5) * Gc);
            be->template launch<K::TailLine, T>(line_blocks(), nb, 1, tb, N);
        }
    }

    // The gain term of this shard from the spectra in fhat (and fhat2 for the bilinear form: the conj(alpha) operand) into qhat.
    // symmetric (one distribution, fhat2 given): every chunk runs a second pass with the two spectra exchanged, whose segment
    // sums and slabs are the entries slab_count + i of slab_sym / pseg_sym; KC, the reduce and the fused tail then cover 2 x slab_count entries, so
    // qhat = gain_hat[g,f] + gain_hat[f,g] in one fixed order.
    // pairs (the batched two-operand forms, collide_pairs): the spectra of the nb members' operands, each with its member stride
    // (0: one spectrum that every member reads); the kernels that read a spectrum then take their batched parameter types, and
    // fhat2 is not read.  The member stride of the symmetric form's slabs and segment sums is 2 x slab_count x G.
    struct OperandSpectra {
        const cx<T>* a;       // the alpha operand (g_hat)
        const cx<T>* b;       // the conj(alpha) operand (f_hat)
        size_t a_bstride, b_bstride;
    };
    void gain_spectra(int nb, bool do_reduce, const cx<T>* fhat2, bool symmetric = false, const OperandSpectra* pairs = nullptr) {
        const int N = plan.N;
        const double Gc = (double)plan.G() * cbytes() * nb;
        const size_t G = plan.G();
        const int n_pass = symmetric ? 2 : 1;
        const size_t a_bs = cap * (size_t)a_planes * N * N, s_bs = (size_t)n_pass * (slab_count ? slab_count : 1) * G;
        const size_t r_bs = cap * r_per_dir();
        const double hfrac = (double)a_planes / N;                 // share of A' actually stored
        cx<T>* const slab = symmetric ? slab_sym : this->slab;       // the symmetric form's own slabs and segment sums
        cx<T>* const pseg = symmetric ? pseg_sym : this->pseg;
        const size_t n_slabs = slab_count * (size_t)n_pass;
        for (const Chunk& c : plan.chunks) for (int pass = 0; pass < n_pass; ++pass) {
            const cx<T>* fa = pass ? fhat2 : fhat;               // the alpha operand's spectrum
            const cx<T>* fb = pass ? fhat : fhat2;               // the conj(alpha) operand's (null: Q(f,f))
            size_t fa_bs = G, fb_bs = G;
            if (pairs) {
                fa = pass ? pairs->b : pairs->a; fa_bs = pass ? pairs->b_bstride : pairs->a_bstride;
                fb = pass ? pairs->a : pairs->b; fb_bs = pass ? pairs->a_bstride : pairs->b_bstride;
            }
            const int seg0 = c.seg0 + pass * (int)slab_count;
            // KA's parallelism is planes x direction groups: keep >= 2 workgroups per CU when only N/2 + 1 planes run
            const int tw_ = target_workgroups(N, max_batch);
            // one resident wave of workgroups, except at N = 64: two rounds of half-length workgroups let the CUs that
            // finish early take more of them (measured, same box, alternating builds: KA 3.25 - 3.28 -> 3.17 - 3.20 ms at
            // config 4, 0.99 - 1.00 -> 0.98 ms at config 3, no change at N = 128: profiles/r03_ka_rounds_ab.txt)
#ifdef BFSM_KA_GROUPS_MULT          // A/B builds (tools only): rounds of KA workgroups
            const int ka_rounds = (BFSM_KA_GROUPS_MULT);
#else
            const int ka_rounds = N == 64 ? 2 : 1;
#endif
            const int groups_a = (tw_ / a_planes > 0 ? tw_ / a_planes : 1) * ka_rounds;
            const int per_group_a = (c.n + groups_a - 1) / groups_a;
            // phase tables beyond ~3 MiB do not stay in an XCD's L2 next to the streams: KA touches the rows ahead
            // (N = 64, config 4: 3 x 2.4 MiB of tables, KA 3.88 -> 3.66 ms; N = 128, config 5: 62 -> 52 ms)
            const bool warm = N >= 64 && 3.0 * (double)plan.n_dirs() * N * sizeof(cx<T>) > 3.0 * 1024 * 1024;
            const int ga = (c.n + per_group_a - 1) / per_group_a;
            // Hermitian mode, N = 64: the chunk's 2 c.n Nyquist-row workgroups (KN) ride along as extra rows of KA's grid
            const bool kn_rides = plan.hermitian && kn_rides_along(N);
            const int kn_blocks = kn_rides ? 2 * c.n : 0, kn_rows = (kn_blocks + a_planes - 1) / a_planes;
            GainInvParams<T> ka{fa, a1, a2, phx, phy, phz, tw, c.dir0, c.n, per_group_a, a_bs, a_planes, warm ? 1 : 0};
            be->mark(BFSM_K_GAIN_INV, 2.0 * c.n * Gc * hfrac);
            if (pairs) {                        // batched two-operand forms: a member stride per spectrum
                GainInvBiBatchParams<T> kab{};
                static_cast<GainInvParams<T>&>(kab) = ka;
                kab.fhat2 = fb;
                kab.f_bstride = fa_bs;
                kab.f2_bstride = fb_bs;
                if (kn_rides) {
                    GainInvNyqBiBatchParams<T> kan{kab, rnyq, r_bs, kn_blocks, ga};
                    be->template launch<K::GainInvNyq, T>(a_planes, ga + kn_rows, nb, kan, N);
                } else if (pair_geometry() && !interleaved()) be->template launch<K::GainInvTwo, T>(a_planes, ga, nb, kab, N);
                else be->template launch<K::GainInv, T>(a_planes, ga, nb, kab, N);
            } else if (fb) {                    // two operands: Q(g,f) on faithful handles, Qs(g,f) on every mode
                GainInvBiParams<T> kab{};
                static_cast<GainInvParams<T>&>(kab) = ka;
                kab.fhat2 = fb;
                if (kn_rides) {
                    GainInvNyqBiParams<T> kan{kab, rnyq, r_bs, kn_blocks, ga};
                    be->template launch<K::GainInvNyq, T>(a_planes, ga + kn_rows, nb, kan, N);
                } else if (pair_geometry() && !interleaved()) be->template launch<K::GainInvTwo, T>(a_planes, ga, nb, kab, N);
                else be->template launch<K::GainInv, T>(a_planes, ga, nb, kab, N);
            } else if (kn_rides) {              // KA + guest KN workgroups
                GainInvNyqParams<T> kan{ka, rnyq, r_bs, kn_blocks, ga};
                be->template launch<K::GainInvNyq, T>(a_planes, ga + kn_rows, nb, kan, N);
            } else if (pair_geometry() && !interleaved()) be->template launch<K::GainInvTwo, T>(a_planes, ga, nb, ka, N);
            else be->template launch<K::GainInv, T>(a_planes, ga, nb, ka, N);
            if (!plan.exact_reductions && segment_sums()) {
                // faithful mode: every direction's own forward x transform, the segment sum of P' in registers
                GainLineSumParams<T> kb{{a1, a2, pseg, dirw, segs, tw, c.dir0, seg0, a_bs, s_bs}};
                be->mark(BFSM_K_GAIN_LINE, (2.0 * c.n + c.n_seg) * Gc);
                be->template launch<K::GainLineAcc, T>(line_blocks(), c.n_seg, nb, kb, N);
            } else if (!plan.exact_reductions) {
                const size_t p_bs = interleaved() ? cap * G : a_bs;
                GainLineParams<T> kb{a1, a2, tw, a_bs, pp, p_bs};
                be->mark(BFSM_K_GAIN_LINE, 3.0 * c.n * Gc);
                be->template launch<K::GainLine, T>(line_blocks(), c.n, nb, kb, N);
                GainFwdParams<T> kc{pp, slab, dirw, segs, tw, c.dir0, seg0, p_bs, s_bs};
                be->mark(BFSM_K_GAIN_FWD, 1.0 * c.n * Gc);
                be->template launch<K::GainFwd, T>(N, c.n_seg, nb, kc, N);
            } else if (!plan.hermitian) {
                GainLineAccParams<T> kb{a1, a2, pseg, dirw, segs, tw, c.dir0, seg0, a_bs, s_bs};
                be->mark(BFSM_K_GAIN_LINE, (2.0 * c.n + c.n_seg) * Gc);
                be->template launch<K::GainLineAcc, T>(line_blocks(), c.n_seg, nb, kb, N);
            } else {
                if (!kn_rides) {
                    NyqRowsParams<T> kn{fa, rnyq, phx, phy, phz, tw, c.dir0, r_bs};
                    const int npl = line_npl(N), ncol = 2 * (N / 2 - 1);
                    be->mark(BFSM_K_GAIN_INV, 0.0);
                    if (pairs) {
                        NyqRowsBiBatchParams<T> knb{};
                        static_cast<NyqRowsParams<T>&>(knb) = kn;
                        knb.fhat2 = fb;
                        knb.f_bstride = fa_bs;
                        knb.f2_bstride = fb_bs;
                        be->template launch<K::NyqRows, T>((ncol + npl - 1) / npl, 2 * c.n, nb, knb, N);
                    } else if (fb) {
                        NyqRowsBiParams<T> knb{};
                        static_cast<NyqRowsParams<T>&>(knb) = kn;
                        knb.fhat2 = fb;
                        be->template launch<K::NyqRows, T>((ncol + npl - 1) / npl, 2 * c.n, nb, knb, N);
                    } else be->template launch<K::NyqRows, T>((ncol + npl - 1) / npl, 2 * c.n, nb, kn, N);
                }
                GainLineAccHParams<T> kb{a1, a2, rnyq, pseg, dirw, segs, tw, c.dir0, seg0, a_bs, s_bs, r_bs};
                be->mark(BFSM_K_GAIN_LINE, (2.0 * c.n * hfrac + c.n_seg) * Gc);
                be->template launch<K::GainLineAccH, T>(line_blocks(), c.n_seg, nb, kb, N);
            }
        }
        if (segment_sums() && slab_count) {   // one forward tile pass per segment, all chunks at once
            GainFwdParams<T> kc{pseg, slab, ones, segs_unit, tw, 0, 0, s_bs, s_bs};
            be->mark(BFSM_K_GAIN_FWD, 1.0 * (double)n_slabs * Gc);
            be->template launch<K::GainFwd, T>(N, (int)n_slabs, nb, kc, N);
        }
        if (do_reduce) {
            ReduceParams<T> kr{slab, qhat, beta1, segs, (int)n_slabs, plan.n2stride, s_bs};
            be->mark(BFSM_K_REDUCE, ((double)n_slabs + 1.0) * Gc);
            be->template launch<K::Reduce, T>((int)((plan.G() + 255) / 256), nb, 1, kr, N);
        }
    }

    // Loss term + final inverse transforms + combine  (CUDABoltzmannOperator.cu:193-216)
    // with_loss = false: Q = Re IFFT(qhat) only -- the partial result a rank contributes when the caller sums Q
    // itself (half the bytes of summing Q_hat) and another rank adds the loss term.
    // from_slabs = true: the slab reduce is fused into the first tail kernel (after gain_partial(.., false)).
    // loss_hat (bilinear form): the spectrum the loss term convolves (f_hat); f_dev is then g, which multiplies it.
    // nu_dev (gain / loss split, bfsm_collide_split*): Q_dev = Re IFFT(qhat), the gain alone, and with_loss adds
    // nu_dev = Re IFFT(beta2 f_hat / G), the collision frequency, instead of subtracting its product with f; f_dev is not read.
    void finish(double* Q_dev, const double* f_dev, bool with_loss = true, int nb = 1, bool from_slabs = false,
                const cx<T>* loss_hat = nullptr, double* nu_dev = nullptr) {
        const int N = plan.N;
        const double Gc = (double)plan.G() * cbytes() * nb;
        const size_t s_bs = (slab_count ? slab_count : 1) * plan.G();
        TailInvParams<T> ta{qhat, loss_hat ? loss_hat : fhat, beta2, tg, (long long)(tl - tg), tw, slab, beta1, segs, from_slabs ? (int)slab_count : -1,
                            plan.n2stride, s_bs};
        be->mark(BFSM_K_TAIL, ((with_loss ? 4.0 : 2.0) + (from_slabs ? (double)slab_count - 1.0 : 0.0)) * Gc);
        be->template launch<K::TailInv, T>(N, with_loss ? 2 : 1, nb, ta, N);
        TailLineParams<T> tb{tg, tl, f_dev, Q_dev, tw, with_loss ? 1 : 0};
        be->mark(BFSM_K_TAIL, (with_loss ? 3.0 : 1.5) * Gc);
        if (nu_dev && with_loss) {     // two complex arrays read, two real ones written: the bytes of the combined form
            TailLineSplitParams<T> ts{};
            static_cast<TailLineParams<T>&>(ts) = tb;
            ts.f = nullptr;
            ts.nu = nu_dev;
            be->template launch<K::TailLine, T>(line_blocks(), nb, 1, ts, N);
        } else be->template launch<K::TailLine, T>(line_blocks(), nb, 1, tb, N);
    }

    // nu = Re IFFT(beta2 f_hat / G) alone (bfsm_loss_rate_async): F1, the loss plane of the first tail kernel, then the
    // gain-only tail line on that array.  No gain work; the direction shard plays no part.
    void loss_rate(double* nu_dev, const double* f_dev, int nb = 1) {
        const int N = plan.N;
        const double Gc = (double)plan.G() * cbytes() * nb;
        spectrum(f_dev, fhat, nb);
        TailInvLossParams<T> ta{{nullptr, fhat, beta2, tg, (long long)(tl - tg), tw, nullptr, nullptr, nullptr, -1, plan.n2stride, 0}};
        be->mark(BFSM_K_TAIL, 2.0 * Gc);
        be->template launch<K::TailInv, T>(N, 1, nb, ta, N);
        TailLineParams<T> tb{tl, tl, nullptr, nu_dev, tw, 0};
        be->mark(BFSM_K_TAIL, 1.5 * Gc);
        be->template launch<K::TailLine, T>(line_blocks(), nb, 1, tb, N);
    }

    // In-place batched 3-D transform on user data (bfsm_fft3d)
    int fft3d(cx<T>* data, int batch, int sign) {
        const int N = plan.N;
        LineParams<T> p{data, data, tw};
        if (sign < 0) {
            be->mark(-1, 0);
            be->template launch<K::TileFwd, T>(N, batch, 1, p, N);
            be->mark(-1, 0);
            be->template launch<K::LineFwd, T>(line_blocks(), batch, 1, p, N);
        } else {
            be->mark(-1, 0);
            be->template launch<K::LineInv, T>(line_blocks(), batch, 1, p, N);
            be->mark(-1, 0);
            be->template launch<K::TileInv, T>(N, batch, 1, p, N);
        }
        return BFSM_OK;
    }
};

// SURVEY.md 8(d) model for this shard, always in FULL quadrature directions (3 FFTs per direction, read + write each)
inline double alg_bytes_per_eval(const PlanInfo& p) {
    const double c = p.precision == BFSM_F64 ? 16.0 : 8.0;
    return (6.0 * (double)(p.full_end - p.full_begin) + 9.0) * (double)p.G() * c;
}

// Bytes the launch sequence actually moves (model).  Faithful mode: 4 array passes per direction (KA writes A1', A2', the
// x-line kernel reads them) + 4 per segment (segment sum written and read, slab written and read); 6 per direction + 2 per
// segment on the per-direction route (P'_d written and read back).  Exact-reduction mode: the same 4 + 4 per EFFECTIVE
// direction and segment.
inline double moved_bytes_per_eval(const PlanInfo& p) {
    const double c = p.precision == BFSM_F64 ? 16.0 : 8.0;
    const double G = (double)p.G(), n = (double)p.n_dirs(), sg = (double)p.segs.size();
    // size-generic path: one pass per axis (or x + a fused (y,z) plane pass), pointwise steps fused on the load side
    if (p.N == 0) return ((double)p.gen_moves * n + 2.0 * p.gen_slabs + (p.gen_plane ? 18.0 : 27.0)) * G * c;
    if (!p.exact_reductions) {
        const bool sums = p.precision == BFSM_F64 ? kb_sums_segments_n<double>(p.N) : kb_sums_segments_n<float>(p.N);
        return sums ? (4.0 * n + 4.0 * sg + 9.0) * G * c : (6.0 * n + 2.0 * sg + 9.0) * G * c;
    }
    const double h = p.hermitian ? (double)(p.N / 2 + 1) / p.N : 1.0;
    return (4.0 * n * h + 4.0 * sg + 9.0) * G * c;
}

}  // namespace bfsm
