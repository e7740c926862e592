// bfsm_conserve.hpp -- conservative projection of Q (BFSM_FLAG_CONSERVE, bfsm_conserve_async).
//
// The discrete Q of the Fourier-spectral method does not conserve the collision invariants: its sums against 1, v and |v|^2
// over the grid sit at truncation level.  Gamba & Tharkabhushanam (J. Comput. Phys. 2009) replace Q by its L2-orthogonal
// projection onto the grid functions whose discrete mass, momentum and energy vanish.  With the basis
//     psi0 = 1, psi1 = vx, psi2 = vy, psi3 = vz, psi4 = |v|^2 - c,   c = (1/G) sum_i |v_i|^2,
// which is orthogonal on the symmetric grid v_a(i) = -L + (i + 1/2) Delta_a, the projection is
//     lambda_k = <psi_k, Q> / <psi_k, psi_k>,   PQ = Q - sum_k lambda_k psi_k      (<a,b> = sum over the G points).
// P is a fixed linear map: it commutes with direction shards, batches and the gain / loss split.  Always fp64 (Q is double at
// the boundary), whatever the transform precision of the handle.
//
// Kernels (256 threads, 16-byte loads of two neighbouring points along z, coordinates from the index, no tables):
//   CK::Moments  grid (W, n_batch): workgroup w sums the five moments over its contiguous range of point pairs, reduces them
//                with a fixed-order LDS tree and writes part[member][w][5];
//   CK::Apply    grid (W, n_batch): every workgroup sums the W partials of its member in the same fixed order (so all get
//                bitwise the same lambda) and subtracts sum_k lambda_k psi_k over its range;
//   CK::Small    grid (1, n_batch), G <= CONS_SMALL_G: one workgroup per member, the member's pairs held in registers (up to
//                CONS_REG per thread; beyond that re-read, L2-warm): read, reduce, solve, write in one launch.
// W depends on G only (never on the device), the order of every sum is fixed and there are no atomics: results are bitwise
// reproducible, and member i of a batch is bitwise the single evaluation of member i.
#pragma once
#include <cmath>
#include <string>

#include "../../include/bfsm.h"
#include "bfsm_core.hpp"

namespace bfsm {

constexpr int CONS_THREADS = 256;
constexpr int CONS_MAX_W = 128;     // moment workgroups per member at most
constexpr int CONS_PAIRS_PER_THREAD = 8;   // W = ceil(pairs / (CONS_THREADS * this)), capped at CONS_MAX_W
constexpr int CONS_REG = 8;         // pairs per thread the one-launch form keeps in registers
#ifndef BFSM_CONS_SMALL_G
#define BFSM_CONS_SMALL_G 4096      // G at or below which the one-launch form is used
#endif
constexpr long long CONS_SMALL_G = BFSM_CONS_SMALL_G;
constexpr size_t CONS_LDS_BYTES = 5 * CONS_THREADS * sizeof(double);

enum class CK { Moments, Apply, Small };

struct ConsParams {
    double* Q;            // [n_batch][G]
    double* part;         // [n_batch][W][5] moment partials
    unsigned nz, ny;      // extents of the two inner axes
    unsigned pairs;       // G / 2 (every extent is even)
    unsigned chunk;       // pairs per workgroup
    int W;                // workgroups per member (CK::Moments / CK::Apply)
    double L, dx, dy, dz; // v_a(i) = -L + (i + 1/2) d_a
    double c;             // (1/G) sum_i |v_i|^2
    double inv0, inv1, inv2, inv3, inv4;   // 1 / <psi_k, psi_k>
};

// the coordinates of the pair starting at point 2 q of a member: vx, vy shared, vz of the two points
struct ConsPoint {
    double vx, vy, vz0, vz1, e0, e1;   // e = |v|^2 - c
};
BFSM_HD ConsPoint cons_point(const ConsParams& p, unsigned q) {
    const unsigned idx = 2u * q, k = idx % p.nz, row = idx / p.nz, j = row % p.ny, i = row / p.ny;
    ConsPoint o;
    o.vx = -p.L + ((double)i + 0.5) * p.dx;
    o.vy = -p.L + ((double)j + 0.5) * p.dy;
    o.vz0 = -p.L + ((double)k + 0.5) * p.dz;
    o.vz1 = -p.L + ((double)k + 1.5) * p.dz;
    const double base = o.vx * o.vx + o.vy * o.vy - p.c;
    o.e0 = base + o.vz0 * o.vz0;
    o.e1 = base + o.vz1 * o.vz1;
    return o;
}

BFSM_HD void cons_accumulate(const ConsParams& p, unsigned q, cx<double> v, double* s) {
    const ConsPoint o = cons_point(p, q);
    const double m = v.x + v.y;
    s[0] += m;
    s[1] += o.vx * m;
    s[2] += o.vy * m;
    s[3] += o.vz0 * v.x + o.vz1 * v.y;
    s[4] += o.e0 * v.x + o.e1 * v.y;
}

BFSM_HD cx<double> cons_subtract(const ConsParams& p, unsigned q, cx<double> v, const double* lam) {
    const ConsPoint o = cons_point(p, q);
    const double lin = lam[0] + lam[1] * o.vx + lam[2] * o.vy;
    v.x -= lin + lam[3] * o.vz0 + lam[4] * o.e0;
    v.y -= lin + lam[3] * o.vz1 + lam[4] * o.e1;
    return v;
}

// Fixed-order LDS tree over the workgroup: the five totals end in red[k * CONS_THREADS] (red = the LDS base), visible to
// every thread after the final barrier.
template <class Ctx>
BFSM_HD void cons_block_sum(const double* s, Ctx& ctx) {
    double* red = ctx.template lds<double>();
    const int t = ctx.tid();
    for (int k = 0; k < 5; ++k) red[k * CONS_THREADS + t] = s[k];
    ctx.sync();
    for (int h = CONS_THREADS / 2; h > 0; h >>= 1) {
        if (t < h)
            for (int k = 0; k < 5; ++k) red[k * CONS_THREADS + t] += red[k * CONS_THREADS + t + h];
        ctx.sync();
    }
}

BFSM_HD void cons_lambda(const ConsParams& p, const double* sum, double* lam) {
    lam[0] = sum[0] * p.inv0;
    lam[1] = sum[1] * p.inv1;
    lam[2] = sum[2] * p.inv2;
    lam[3] = sum[3] * p.inv3;
    lam[4] = sum[4] * p.inv4;
}

template <class Ctx>
BFSM_HD void body_cons_moments(const ConsParams& p, Ctx& ctx) {
    const int b = ctx.by(), w = ctx.bx(), t = ctx.tid();
    const cx<double>* row = reinterpret_cast<const cx<double>*>(p.Q + (size_t)b * 2 * p.pairs);
    const unsigned p0 = (unsigned)w * p.chunk, p1 = p0 + p.chunk < p.pairs ? p0 + p.chunk : p.pairs;
    double s[5] = {0, 0, 0, 0, 0};
    for (unsigned q = p0 + (unsigned)t; q < p1; q += CONS_THREADS)
        cons_accumulate(p, q, ctx.template ld_at<false>(row, q * (unsigned)sizeof(cx<double>)), s);
    cons_block_sum(s, ctx);
    const double* red = ctx.template lds<double>();
    if (t < 5) p.part[((size_t)b * p.W + w) * 5 + t] = red[t * CONS_THREADS];
}

template <class Ctx>
BFSM_HD void body_cons_apply(const ConsParams& p, Ctx& ctx) {
    const int b = ctx.by(), w = ctx.bx(), t = ctx.tid();
    double* red = ctx.template lds<double>();
    if (t < 5) {          // the W partials of this member, in the same order in every workgroup
        const double* pp = p.part + (size_t)b * p.W * 5 + t;
        double a = 0;
        for (int i = 0; i < p.W; ++i) a += pp[(size_t)i * 5];
        red[t] = a;
    }
    ctx.sync();
    const double sum[5] = {red[0], red[1], red[2], red[3], red[4]};
    double lam[5];
    cons_lambda(p, sum, lam);
    cx<double>* row = reinterpret_cast<cx<double>*>(p.Q + (size_t)b * 2 * p.pairs);
    const unsigned p0 = (unsigned)w * p.chunk, p1 = p0 + p.chunk < p.pairs ? p0 + p.chunk : p.pairs;
    for (unsigned q = p0 + (unsigned)t; q < p1; q += CONS_THREADS) {
        const unsigned off = q * (unsigned)sizeof(cx<double>);
        ctx.template st_at<false>(row, off, cons_subtract(p, q, ctx.template ld_at<false>(row, off), lam));
    }
}

template <class Ctx>
BFSM_HD void body_cons_small(const ConsParams& p, Ctx& ctx) {
    const int b = ctx.by(), t = ctx.tid();
    cx<double>* row = reinterpret_cast<cx<double>*>(p.Q + (size_t)b * 2 * p.pairs);
    constexpr unsigned SZ = (unsigned)sizeof(cx<double>);
    cx<double> keep[CONS_REG];
    double s[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < CONS_REG; ++m) {
        const unsigned q = (unsigned)t + (unsigned)m * CONS_THREADS;
        keep[m] = cx<double>{0, 0};
        if (q < p.pairs) {
            keep[m] = ctx.template ld_at<false>(row, q * SZ);
            cons_accumulate(p, q, keep[m], s);
        }
    }
    for (unsigned q = (unsigned)t + CONS_REG * CONS_THREADS; q < p.pairs; q += CONS_THREADS)
        cons_accumulate(p, q, ctx.template ld_at<false>(row, q * SZ), s);
    cons_block_sum(s, ctx);
    const double* red = ctx.template lds<double>();
    const double sum[5] = {red[0], red[CONS_THREADS], red[2 * CONS_THREADS], red[3 * CONS_THREADS], red[4 * CONS_THREADS]};
    double lam[5];
    cons_lambda(p, sum, lam);
#pragma unroll
    for (int m = 0; m < CONS_REG; ++m) {
        const unsigned q = (unsigned)t + (unsigned)m * CONS_THREADS;
        if (q < p.pairs) ctx.template st_at<false>(row, q * SZ, cons_subtract(p, q, keep[m], lam));
    }
    for (unsigned q = (unsigned)t + CONS_REG * CONS_THREADS; q < p.pairs; q += CONS_THREADS)
        ctx.template st_at<false>(row, q * SZ, cons_subtract(p, q, ctx.template ld_at<false>(row, q * SZ), lam));
}

// the body of kernel `kind` on one workgroup (a macro for the reason given at BFSM_RUN_BODY, bfsm_pipeline.hpp)
#define BFSM_RUN_CONS_BODY(kind, prm, ctx)                           \
    if constexpr (kind == CK::Moments) body_cons_moments(prm, ctx);  \
    else if constexpr (kind == CK::Apply) body_cons_apply(prm, ctx); \
    else if constexpr (kind == CK::Small) body_cons_small(prm, ctx);

// Host side: the constants (long double, at bfsm_create) and the launch sequence.  Beside the pipelines, not inside them:
// the entry points call apply() on the same backend and stream after the pipeline's launches.  `Backend` supplies alloc /
// release / mark and  template <CK kind> void launch_cons(int grid_x, int grid_y, const ConsParams&).
template <class Backend>
struct Conserver {
    Backend* be = nullptr;
    ConsParams prm{};
    int max_batch = 1;
    bool small = false;
    size_t G = 0;

    int init(const bfsm_desc& d, Backend* backend, std::string& err) {
        be = backend;
        G = (size_t)d.nvx * d.nvy * d.nvz;
        max_batch = d.max_batch > 1 ? d.max_batch : 1;
        const int n[3] = {d.nvx, d.nvy, d.nvz};
        const long double L = (long double)d.L;
        long double s1[3], s2[3], s3[3], s4[3], a1[3], a3[3];   // sums of v, v^2, v^3, v^4, |v|, |v|^3 along each axis
        for (int a = 0; a < 3; ++a) {
            s1[a] = s2[a] = s3[a] = s4[a] = a1[a] = a3[a] = 0;
            const long double da = 2 * L / n[a];
            for (int i = 0; i < n[a]; ++i) {
                const long double v = -L + ((long double)i + 0.5L) * da, v2 = v * v;
                s1[a] += v; s2[a] += v2; s3[a] += v2 * v; s4[a] += v2 * v2;
                a1[a] += fabsl(v); a3[a] += fabsl(v2 * v);
            }
            // every off-diagonal Gram entry of the basis is a product / sum of terms holding an odd sum of one axis
            if (fabsl(s1[a]) > 1e-12L * a1[a] || fabsl(s3[a]) > 1e-12L * a3[a]) {
                err = "conservative projection: the velocity grid is not symmetric (odd moments do not vanish)";
                return BFSM_ERR_INVALID;
            }
        }
        const long double Gl = (long double)G, nx = n[0], ny = n[1], nz = n[2];
        const long double sv2 = ny * nz * s2[0] + nx * nz * s2[1] + nx * ny * s2[2];      // sum_i |v_i|^2
        const long double c = sv2 / Gl;
        // sum_i |v_i|^4 = sum (a + b + d)^2 with a = vx^2, b = vy^2, d = vz^2 separable
        const long double sv4 = ny * nz * s4[0] + nx * nz * s4[1] + nx * ny * s4[2] +
                                2 * (nz * s2[0] * s2[1] + ny * s2[0] * s2[2] + nx * s2[1] * s2[2]);
        const long double g4 = sv4 - Gl * c * c;                                            // <psi4, psi4>
        prm.nz = (unsigned)d.nvz;
        prm.ny = (unsigned)d.nvy;
        prm.pairs = (unsigned)(G / 2);
        long long w = ((long long)prm.pairs + CONS_THREADS * CONS_PAIRS_PER_THREAD - 1) / (CONS_THREADS * CONS_PAIRS_PER_THREAD);
        if (w > CONS_MAX_W) w = CONS_MAX_W;
        if (w < 1) w = 1;
        prm.chunk = (unsigned)((prm.pairs + w - 1) / w);
        prm.W = (int)((prm.pairs + prm.chunk - 1) / prm.chunk);
        prm.L = d.L;
        prm.dx = (double)(2 * L / n[0]);
        prm.dy = (double)(2 * L / n[1]);
        prm.dz = (double)(2 * L / n[2]);
        prm.c = (double)c;
        prm.inv0 = (double)(1.0L / Gl);
        prm.inv1 = (double)(1.0L / (ny * nz * s2[0]));
        prm.inv2 = (double)(1.0L / (nx * nz * s2[1]));
        prm.inv3 = (double)(1.0L / (nx * ny * s2[2]));
        prm.inv4 = (double)(1.0L / g4);
        small = (long long)G <= CONS_SMALL_G;
        prm.part = (double*)be->alloc((size_t)max_batch * prm.W * 5 * sizeof(double));
        if (!prm.part) { err = "device allocation failed"; return BFSM_ERR_NOMEM; }
        return BFSM_OK;
    }

    // Q (n_batch consecutive members of G doubles, device) := P Q, in place
    void apply(double* Q, int nb) {
        ConsParams p = prm;
        p.Q = Q;
        const double bytes = (double)G * sizeof(double) * nb;
        if (small) {
            be->mark(BFSM_K_TAIL, 2.0 * bytes);
            be->template launch_cons<CK::Small>(1, nb, p);
            return;
        }
        be->mark(BFSM_K_TAIL, 1.0 * bytes);
        be->template launch_cons<CK::Moments>(p.W, nb, p);
        be->mark(BFSM_K_TAIL, 2.0 * bytes);
        be->template launch_cons<CK::Apply>(p.W, nb, p);
    }

    // bytes one single-distribution projection moves (model): read + write, plus the second read of the two-launch form
    double moved_bytes() const { return (small ? 2.0 : 3.0) * (double)G * sizeof(double); }

    void destroy() {
        if (be && prm.part) be->release(prm.part);
        prm.part = nullptr;
    }
};

}  // namespace bfsm
