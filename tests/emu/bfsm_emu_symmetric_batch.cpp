// bfsm_emu_symmetric_batch.cpp -- TEST HARNESS ONLY.  The host lock-step emulator of bfsm_emu.cpp, plus the batched two-operand
// forms: the plan and launch sequence of bfsm_collide_symmetric_batch_partial_async / bfsm_collide_bilinear_batch_partial_async
// (bfsm_calls.hpp, collide_pairs: Pipeline::collide_pairs on the fused cubes, member by member on every other box), run by the
// emulated kernel bodies on a backend that also counts the launches per kernel kind.  Built into its own shared library by
// tests/test_emu_symmetric_batch.py with the flags of tests/emu/Makefile; tests/emu/symmetric_batch_sanitize_main.cpp includes
// it for its stand-alone sanitizer run.
#include "bfsm_emu.cpp"

namespace emu {

struct CountBackend : EmuBackend {
    int launches[64] = {};                 // [kind]: launches by bfsm::K; [32 + kind]: their grid.y summed (the members an input
                                           // transform's launches cover: F1's grid is (N | line blocks, members, 1))
    template <bfsm::K kind, typename T, class P>
    void launch(int gx, int gy, int gz, const P& prm, int N) {
        if (gx > 0 && gy > 0 && gz > 0) { ++launches[(int)kind]; launches[32 + (int)kind] += gy; }
        EmuBackend::launch<kind, T>(gx, gy, gz, prm, N);
    }
};

// with_pipeline of bfsm_emu.cpp on the counting backend; launches (may be null) receives the 64 counts
template <class F>
int with_counting_pipeline(const bfsm_desc* d, int n_batch, int* launches, F&& fn) {
    auto run = [&](auto p) {
        CountBackend be;
        std::string err;
        int rc = p.init(*d, &be, err);
        if (!rc && (n_batch < 1 || n_batch > p.max_batch)) rc = BFSM_ERR_INVALID;
        if (!rc) fn(p);
        p.destroy();
        if (launches) for (int i = 0; i < 64; ++i) launches[i] = be.launches[i];
        return rc ? rc : (be.failed ? 99 : 0);
    };
    if (bfsm::fused_grid(*d))
        return d->precision == BFSM_F64 ? run(bfsm::Pipeline<double, CountBackend>()) : run(bfsm::Pipeline<float, CountBackend>());
    return d->precision == BFSM_F64 ? run(bfsm::GenericPipeline<double, CountBackend>()) : run(bfsm::GenericPipeline<float, CountBackend>());
}

// the argument rules of the C entry points that do not need a device
inline int pairs_args(const bfsm_desc* d, const double* g, const double* f, const double* Q, int share, int symmetric) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    if (!g || !f || !Q) return BFSM_ERR_INVALID;
    if (share != BFSM_SHARE_NONE && share != BFSM_SHARE_G && share != BFSM_SHARE_F) return BFSM_ERR_INVALID;
    if (!symmetric && (d->flags & BFSM_FLAG_EXACT_REDUCTIONS)) return BFSM_ERR_UNSUPPORTED;
    return BFSM_OK;
}

}  // namespace emu

extern "C" {

// Emulated bfsm_collide_symmetric_batch_partial_async (symmetric != 0) / bfsm_collide_bilinear_batch_partial_async on host arrays
int bfsm_emu_collide_pairs(const bfsm_desc* d, const double* g, const double* f, double* Q, int n_batch, int share, int with_loss,
                           int symmetric, int* launches) {
    int rc = emu::pairs_args(d, g, f, Q, share, symmetric);
    if (rc) return rc;
    return emu::with_counting_pipeline(d, n_batch, launches, [&](auto& p) {
        bfsm::collide_pairs(p, Q, g, f, n_batch, share, with_loss != 0, symmetric != 0);
    });
}

// The single call on a handle of the same descriptor (max_batch included): bfsm_collide_symmetric_partial_async /
// bfsm_collide_bilinear_partial_async
int bfsm_emu_collide_pair_single(const bfsm_desc* d, const double* g, const double* f, double* Q, int with_loss, int symmetric,
                                 int* launches) {
    int rc = emu::pairs_args(d, g, f, Q, BFSM_SHARE_NONE, symmetric);
    if (rc) return rc;
    return emu::with_counting_pipeline(d, 1, launches, [&](auto& p) {
        if (symmetric) bfsm::collide_symmetric(p, Q, g, f, with_loss != 0);
        else p.collide_bilinear(Q, g, f, with_loss != 0);
    });
}

}  // extern "C"
