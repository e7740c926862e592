// bfsm_calls.hpp -- what each entry point of include/bfsm.h launches, stated once: sequences of the primitives of Pipeline
// (bfsm_pipeline.hpp) and GenericPipeline (bfsm_generic.hpp), as function templates over the pipeline type.  Pure C++17, no
// HIP: bfsm_hip.hip calls them from its extern "C" bodies, the host emulator and its launch recorder (tests/emu) call the same
// functions, so a test of a sequence is a test of the library's.
#pragma once
#include <cstddef>

namespace bfsm {

// A batch through fn(first member, members): together where the pipeline's launches cover a batch, else one by one
template <class Pipe, class F>
void for_batch(Pipe& p, int n_batch, F&& fn) {
    if (p.batch_together()) fn(0, n_batch);
    else for (int i = 0; i < n_batch; ++i) fn(i, 1);
}

// Q = gain of the shard [- loss] for n_batch distributions (bfsm_collide*_async, bfsm_collide_batch*_async): the
// whole-direction kernels where the handle has them (N = 16, one evaluation), otherwise the gain kernels, then the tail.
// fuse: the slab reduce runs inside the first tail kernel (qhat is not written then); the library passes p.fuse_reduce().
template <class Pipe>
void collide(Pipe& p, double* Q, const double* f, int n_batch, bool with_loss, bool fuse) {
    const size_t G = p.plan.G();
    for_batch(p, n_batch, [&](int i0, int nb) {
        const size_t o = (size_t)i0 * G;
        if (p.small_path(nb)) { p.collide_small(Q + o, f + o, with_loss); return; }
        p.gain_partial(f + o, nb, !fuse);
        p.finish(Q + o, f + o, with_loss, nb, fuse);
    });
}

// The same with the two terms of the tail kept apart (bfsm_collide_split*_async): Qgain = the gain alone and, with_loss,
// nu = the collision frequency.  N = 16 takes the plane-tile pipeline.
template <class Pipe>
void collide_split(Pipe& p, double* Qgain, double* nu, const double* f, int n_batch, bool with_loss, bool fuse) {
    const size_t G = p.plan.G();
    for_batch(p, n_batch, [&](int i0, int nb) {
        const size_t o = (size_t)i0 * G;
        p.gain_partial(f + o, nb, !fuse);
        p.finish(Qgain + o, nullptr, with_loss, nb, fuse, nullptr, with_loss ? nu + o : nullptr);
    });
}

// Qs(g,f) = Q(g,f) + Q(f,g) of the shard [- both loss terms] for one distribution pair (bfsm_collide_symmetric*_async), on every
// kind of handle.  Fused cubes, every mode (Pipeline::collide_symmetric): two gain passes per chunk with the spectra exchanged
// into doubled segment sums and slabs, one KC, one reduce, one three-plane tail; N = 16 takes the plane-tile pipeline.
// Size-generic boxes (GenericPipeline::collide_symmetric): the bilinear gain launches twice, the second pass accumulating onto
// the first one's Q_hat, one tail with both loss terms.
template <class Pipe>
void collide_symmetric(Pipe& p, double* Q, const double* g, const double* f, bool with_loss) {
    p.collide_symmetric(Q, g, f, with_loss);
}

// Member i of Q = Qs(g_i, f_i) (symmetric) or Q(g_i, f_i) of the shard [- the loss terms] for n_batch pairs
// (bfsm_collide_symmetric_batch*_async, bfsm_collide_bilinear_batch_partial_async).  share (BFSM_SHARE_*): g or f is one array that
// every member reads.  Fused cubes (Pipeline::collide_pairs): ONE sequence for the batch -- two spectra passes (a shared operand
// transformed once: n_batch + 1 input transforms), per chunk the gain passes with the batch in the grid, one KC, one reduce (or
// the reduce fused into the tail), one tail; with n_batch = 1 the launches of the single call.  Size-generic boxes: member by
// member through collide_symmetric / collide_bilinear (a shared operand is transformed per member there).
template <class Pipe>
void collide_pairs(Pipe& p, double* Q, const double* g, const double* f, int n_batch, int share, bool with_loss, bool symmetric) {
    if constexpr (Pipe::pair_batches) p.collide_pairs(Q, g, f, n_batch, share, with_loss, symmetric);
    else {
        const size_t G = p.plan.G();
        for (int i = 0; i < n_batch; ++i) {
            const double* gi = g + (share == BFSM_SHARE_G ? 0 : (size_t)i * G);
            const double* fi = f + (share == BFSM_SHARE_F ? 0 : (size_t)i * G);
            if (symmetric) p.collide_symmetric(Q + (size_t)i * G, gi, fi, with_loss);
            else p.collide_bilinear(Q + (size_t)i * G, gi, fi, with_loss);
        }
    }
}

// Bytes the batched symmetric call moves on the fused pipeline (model): n_batch single calls, less the transform of a shared
// operand (3.5 arrays) for every member but one
inline double symmetric_batch_moved_bytes_per_eval(const PlanInfo& p, int n_batch, int share);

// Bytes the symmetric call moves on the fused pipeline (model; the counterpart of moved_bytes_per_eval): per effective direction
// four stored A' arrays written once and read once (two passes of A1', A2'; h = the stored share of the planes, (N/2 + 1)/N on
// Hermitian handles), twice the segment sums and slabs, two transforms of an input and a three-plane tail (9 + 6.5 arrays).
// The per-direction route of the faithful mode moves 12 n + 4 sg.  Two faithful bilinear calls move 2 (4 n_full + 4 sg + 9).
inline double symmetric_moved_bytes_per_eval(const PlanInfo& p) {
    const double c = p.precision == BFSM_F64 ? 16.0 : 8.0;
    const double G = (double)p.G(), n = (double)p.n_dirs(), sg = (double)p.segs.size();
    if (p.N == 0) return (2.0 * (double)p.gen_moves * n + 4.0 * p.gen_slabs + (p.gen_plane ? 28.0 : 42.0)) * G * c;
    const double h = p.hermitian ? (double)(p.N / 2 + 1) / p.N : 1.0;
    const bool sums = p.exact_reductions || (p.precision == BFSM_F64 ? kb_sums_segments_n<double>(p.N) : kb_sums_segments_n<float>(p.N));
    return ((sums ? 8.0 * n * h + 8.0 * sg : 12.0 * n + 4.0 * sg) + 15.5) * G * c;
}

inline double symmetric_batch_moved_bytes_per_eval(const PlanInfo& p, int n_batch, int share) {
    const double c = p.precision == BFSM_F64 ? 16.0 : 8.0;
    const double saved = (p.N != 0 && share != BFSM_SHARE_NONE) ? 3.5 * (double)(n_batch - 1) * (double)p.G() * c : 0.0;
    return (double)n_batch * symmetric_moved_bytes_per_eval(p) - saved;
}

// nu alone (bfsm_loss_rate_async)
template <class Pipe>
void loss_rate(Pipe& p, double* nu, const double* f, int n_batch) {
    const size_t G = p.plan.G();
    for_batch(p, n_batch, [&](int i0, int nb) { p.loss_rate(nu + (size_t)i0 * G, f + (size_t)i0 * G, nb); });
}

}  // namespace bfsm
