// bfsm_moments.hpp -- macroscopic state of f on the device (bfsm_moments_async, bfsm_maxwellian_async).
//
// What a BGK / ES-BGK closure, a penalized (Filbet & Jin, J. Comput. Phys. 2010) or exponential stepper, the H-theorem
// diagnostic and a fluid coupling read from f: with dV = dx dy dz and the grid v_a(i) = -L + (i + 1/2) Delta_a,
//     rho = dV sum f,   m = dV sum v f,   E = dV sum |v|^2 f  (= rho (|u|^2 + 3 T)),   u = m / rho,   T = (E / rho - |u|^2) / 3,
//     H = dV sum_{f > 0} f log f                              (points with f <= 0 contribute 0),
// and the local Maxwellian M[f] = rho (2 pi T)^(-3/2) exp(-|v - u|^2 / 2T) on the grid.  rho = 0 gives u = T = 0.  Always
// fp64 (f is double at the boundary), whatever the transform precision of the handle; f is never written.
//
// Kernels (the conventions of bfsm_conserve.hpp: 256 threads, 16-byte accesses of two neighbouring points along z,
// coordinates from the index, no tables):
//   MK::Sums        grid (W, n_batch): workgroup w sums 1, vx, vy, vz, |v|^2 and log f against f over its contiguous range of
//                   point pairs, reduces them with a fixed-order LDS tree and writes part[member][w][6];
//   MK::Finish      grid (1, n_batch): threads 0..5 add the W partials in index order, thread 0 derives u and T and writes
//                   the member's BFSM_MOM_COUNT doubles;
//   MK::Small       grid (1, n_batch), G <= MOM_SMALL_G: one workgroup reads the member, reduces and writes the row;
//   MK::Maxwellian  grid (W, n_batch): every thread reads rho, u, T of its member from the row and writes M over its range.
//                   A member whose rho or T is not finite and positive gets M = 0 everywhere: the device cannot report an
//                   error, and the other members of the batch are unaffected.
// W depends on G only (never on the device), the order of every sum is fixed and there are no atomics: results are bitwise
// reproducible, and member i of a batch is bitwise the single call on member i.
#pragma once
#include <cmath>
#include <string>

#include "../../include/bfsm.h"
#include "bfsm_core.hpp"

namespace bfsm {

constexpr int MOM_THREADS = 256;
constexpr int MOM_MAX_W = 128;             // workgroups per member at most
constexpr int MOM_PAIRS_PER_THREAD = 8;    // W = ceil(pairs / (MOM_THREADS * this)), capped at MOM_MAX_W
constexpr int MOM_SUMS = 6;                // 1, vx, vy, vz, |v|^2, log f
#ifndef BFSM_MOM_SMALL_G
#define BFSM_MOM_SMALL_G 4096              // G at or below which the one-launch form is used
#endif
constexpr long long MOM_SMALL_G = BFSM_MOM_SMALL_G;
constexpr size_t MOM_LDS_BYTES = MOM_SUMS * MOM_THREADS * sizeof(double);   // 12 KiB

enum class MK { Sums, Finish, Small, Maxwellian };

struct MomParams {
    const double* f;      // [n_batch][G]                      (Sums, Small)
    double* mom;          // [n_batch][BFSM_MOM_COUNT]         (written by Finish / Small, read by Maxwellian)
    double* M;            // [n_batch][G]                      (Maxwellian)
    double* part;         // [n_batch][W][MOM_SUMS] partial sums
    unsigned nz, ny;      // extents of the two inner axes
    unsigned pairs;       // G / 2 (every extent is even)
    unsigned chunk;       // pairs per workgroup
    int W;                // workgroups per member (Sums / Maxwellian)
    double L, dx, dy, dz; // v_a(i) = -L + (i + 1/2) d_a
    double dV;            // dx dy dz
};

// the coordinates of the pair starting at point 2 q of a member: vx, vy shared, vz of the two points
struct MomPoint {
    double vx, vy, vz0, vz1;
};
BFSM_HD MomPoint mom_point(const MomParams& p, unsigned q) {
    const unsigned idx = 2u * q, k = idx % p.nz, row = idx / p.nz, j = row % p.ny, i = row / p.ny;
    MomPoint o;
    o.vx = -p.L + ((double)i + 0.5) * p.dx;
    o.vy = -p.L + ((double)j + 0.5) * p.dy;
    o.vz0 = -p.L + ((double)k + 0.5) * p.dz;
    o.vz1 = -p.L + ((double)k + 1.5) * p.dz;
    return o;
}

BFSM_HD double mom_flogf(double f) { return f > 0.0 ? f * log(f) : 0.0; }

BFSM_HD void mom_accumulate(const MomParams& p, unsigned q, cx<double> v, double* s) {
    const MomPoint o = mom_point(p, q);
    const double m = v.x + v.y, base = o.vx * o.vx + o.vy * o.vy;
    s[0] += m;
    s[1] += o.vx * m;
    s[2] += o.vy * m;
    s[3] += o.vz0 * v.x + o.vz1 * v.y;
    s[4] += (base + o.vz0 * o.vz0) * v.x + (base + o.vz1 * o.vz1) * v.y;
    s[5] += mom_flogf(v.x) + mom_flogf(v.y);
}

// the sums of workgroup range [p0, p1) of member b, thread t's share
template <class Ctx>
BFSM_HD void mom_range_sums(const MomParams& p, int b, unsigned p0, unsigned p1, double* s, Ctx& ctx) {
    const cx<double>* row = reinterpret_cast<const cx<double>*>(p.f + (size_t)b * 2 * p.pairs);
    for (unsigned q = p0 + (unsigned)ctx.tid(); q < p1; q += MOM_THREADS)
        mom_accumulate(p, q, ctx.template ld_at<false>(row, q * (unsigned)sizeof(cx<double>)), s);
}

// Fixed-order LDS tree over the workgroup: the six totals end in red[k * MOM_THREADS] (red = the LDS base), visible to
// every thread after the final barrier.
template <class Ctx>
BFSM_HD void mom_block_sum(const double* s, Ctx& ctx) {
    double* red = ctx.template lds<double>();
    const int t = ctx.tid();
    for (int k = 0; k < MOM_SUMS; ++k) red[k * MOM_THREADS + t] = s[k];
    ctx.sync();
    for (int h = MOM_THREADS / 2; h > 0; h >>= 1) {
        if (t < h)
            for (int k = 0; k < MOM_SUMS; ++k) red[k * MOM_THREADS + t] += red[k * MOM_THREADS + t + h];
        ctx.sync();
    }
}

// the member's row from its six grid sums (one thread)
BFSM_HD void mom_derive(const MomParams& p, const double* sum, double* out) {
    const double rho = p.dV * sum[0], mx = p.dV * sum[1], my = p.dV * sum[2], mz = p.dV * sum[3], E = p.dV * sum[4];
    double ux = 0, uy = 0, uz = 0, T = 0;
    if (rho != 0.0) {
        ux = mx / rho;
        uy = my / rho;
        uz = mz / rho;
        T = (E / rho - (ux * ux + uy * uy + uz * uz)) / 3.0;
    }
    out[BFSM_MOM_RHO] = rho;
    out[BFSM_MOM_MX] = mx;
    out[BFSM_MOM_MY] = my;
    out[BFSM_MOM_MZ] = mz;
    out[BFSM_MOM_E] = E;
    out[BFSM_MOM_UX] = ux;
    out[BFSM_MOM_UY] = uy;
    out[BFSM_MOM_UZ] = uz;
    out[BFSM_MOM_T] = T;
    out[BFSM_MOM_H] = p.dV * sum[5];
}

template <class Ctx>
BFSM_HD void body_mom_sums(const MomParams& p, Ctx& ctx) {
    const int b = ctx.by(), w = ctx.bx(), t = ctx.tid();
    const unsigned p0 = (unsigned)w * p.chunk, p1 = p0 + p.chunk < p.pairs ? p0 + p.chunk : p.pairs;
    double s[MOM_SUMS] = {0, 0, 0, 0, 0, 0};
    mom_range_sums(p, b, p0, p1, s, ctx);
    mom_block_sum(s, ctx);
    const double* red = ctx.template lds<double>();
    if (t < MOM_SUMS) p.part[((size_t)b * p.W + w) * MOM_SUMS + t] = red[t * MOM_THREADS];
}

template <class Ctx>
BFSM_HD void body_mom_finish(const MomParams& p, Ctx& ctx) {
    const int b = ctx.by(), t = ctx.tid();
    double* red = ctx.template lds<double>();
    if (t < MOM_SUMS) {
        const double* pp = p.part + (size_t)b * p.W * MOM_SUMS + t;
        double a = 0;
        for (int i = 0; i < p.W; ++i) a += pp[(size_t)i * MOM_SUMS];
        red[t] = a;
    }
    ctx.sync();
    if (t == 0) mom_derive(p, red, p.mom + (size_t)b * BFSM_MOM_COUNT);
}

template <class Ctx>
BFSM_HD void body_mom_small(const MomParams& p, Ctx& ctx) {
    const int b = ctx.by(), t = ctx.tid();
    double s[MOM_SUMS] = {0, 0, 0, 0, 0, 0};
    mom_range_sums(p, b, 0u, p.pairs, s, ctx);
    mom_block_sum(s, ctx);
    if (t == 0) {
        const double* red = ctx.template lds<double>();
        double sum[MOM_SUMS];
        for (int k = 0; k < MOM_SUMS; ++k) sum[k] = red[k * MOM_THREADS];
        mom_derive(p, sum, p.mom + (size_t)b * BFSM_MOM_COUNT);
    }
}

template <class Ctx>
BFSM_HD void body_mom_maxwellian(const MomParams& p, Ctx& ctx) {
    const int b = ctx.by(), w = ctx.bx(), t = ctx.tid();
    const double* r = p.mom + (size_t)b * BFSM_MOM_COUNT;
    const double rho = r[BFSM_MOM_RHO], ux = r[BFSM_MOM_UX], uy = r[BFSM_MOM_UY], uz = r[BFSM_MOM_UZ], T = r[BFSM_MOM_T];
    const double inf = __builtin_huge_val();
    const bool ok = rho > 0.0 && rho < inf && T > 0.0 && T < inf;      // false for NaN as well
    const double s = 2.0 * 3.14159265358979323846 * (ok ? T : 1.0);
    const double coef = ok ? rho / (s * sqrt(s)) : 0.0, a = ok ? -0.5 / T : 0.0;
    cx<double>* row = reinterpret_cast<cx<double>*>(p.M + (size_t)b * 2 * p.pairs);
    const unsigned p0 = (unsigned)w * p.chunk, p1 = p0 + p.chunk < p.pairs ? p0 + p.chunk : p.pairs;
    for (unsigned q = p0 + (unsigned)t; q < p1; q += MOM_THREADS) {
        cx<double> v{0.0, 0.0};
        if (ok) {
            const MomPoint o = mom_point(p, q);
            const double wx = o.vx - ux, wy = o.vy - uy, w0 = o.vz0 - uz, w1 = o.vz1 - uz, base = wx * wx + wy * wy;
            v.x = coef * exp(a * (base + w0 * w0));
            v.y = coef * exp(a * (base + w1 * w1));
        }
        ctx.template st_at<false>(row, q * (unsigned)sizeof(cx<double>), v);
    }
}

// the body of kernel `kind` on one workgroup (a macro for the reason given at BFSM_RUN_BODY, bfsm_pipeline.hpp)
#define BFSM_RUN_MOM_BODY(kind, prm, ctx)                              \
    if constexpr (kind == MK::Sums) body_mom_sums(prm, ctx);           \
    else if constexpr (kind == MK::Finish) body_mom_finish(prm, ctx);  \
    else if constexpr (kind == MK::Small) body_mom_small(prm, ctx);    \
    else if constexpr (kind == MK::Maxwellian) body_mom_maxwellian(prm, ctx);

// Host side: the constants (at bfsm_create) and the launch sequences.  Beside the pipelines, like Conserver.  `Backend`
// supplies alloc / release / mark and  template <MK kind> void launch_mom(int grid_x, int grid_y, const MomParams&).
template <class Backend>
struct Macroscopic {
    Backend* be = nullptr;
    MomParams prm{};
    int max_batch = 1;
    bool small = false;
    size_t G = 0;

    int init(const bfsm_desc& d, Backend* backend, std::string& err) {
        be = backend;
        G = (size_t)d.nvx * d.nvy * d.nvz;
        max_batch = d.max_batch > 1 ? d.max_batch : 1;
        prm.nz = (unsigned)d.nvz;
        prm.ny = (unsigned)d.nvy;
        prm.pairs = (unsigned)(G / 2);
        long long w = ((long long)prm.pairs + MOM_THREADS * MOM_PAIRS_PER_THREAD - 1) / (MOM_THREADS * MOM_PAIRS_PER_THREAD);
        if (w > MOM_MAX_W) w = MOM_MAX_W;
        if (w < 1) w = 1;
        prm.chunk = (unsigned)((prm.pairs + w - 1) / w);
        prm.W = (int)((prm.pairs + prm.chunk - 1) / prm.chunk);
        const long double L = (long double)d.L;
        prm.L = d.L;
        prm.dx = (double)(2 * L / d.nvx);
        prm.dy = (double)(2 * L / d.nvy);
        prm.dz = (double)(2 * L / d.nvz);
        prm.dV = (double)((2 * L / d.nvx) * (2 * L / d.nvy) * (2 * L / d.nvz));
        small = (long long)G <= MOM_SMALL_G;
        prm.part = (double*)be->alloc((size_t)max_batch * prm.W * MOM_SUMS * sizeof(double));
        if (!prm.part) { err = "device allocation failed"; return BFSM_ERR_NOMEM; }
        return BFSM_OK;
    }

    // mom[i][0..BFSM_MOM_COUNT) := the row of f[i], i < nb (device arrays)
    void moments(double* mom, const double* f, int nb) {
        MomParams p = prm;
        p.f = f;
        p.mom = mom;
        be->mark(BFSM_K_TAIL, moved_bytes() * nb);
        if (small) {
            be->template launch_mom<MK::Small>(1, nb, p);
            return;
        }
        be->template launch_mom<MK::Sums>(p.W, nb, p);
        be->mark(BFSM_K_TAIL, 0.0);
        be->template launch_mom<MK::Finish>(1, nb, p);
    }

    // M[i] := the Maxwellian of row mom[i] on the grid, i < nb (device arrays; reads indices RHO, UX..UZ, T of a row)
    void maxwellian(double* M, const double* mom, int nb) {
        MomParams p = prm;
        p.M = M;
        p.mom = const_cast<double*>(mom);
        be->mark(BFSM_K_TAIL, moved_bytes() * nb);
        be->template launch_mom<MK::Maxwellian>(p.W, nb, p);
    }

    // bytes one member moves (model): moments reads f once, maxwellian writes M once
    double moved_bytes() const { return (double)G * sizeof(double); }

    void destroy() {
        if (be && prm.part) be->release(prm.part);
        prm.part = nullptr;
    }
};

}  // namespace bfsm
