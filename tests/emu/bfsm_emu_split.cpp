// bfsm_emu_split.cpp -- TEST HARNESS ONLY.  The host lock-step emulator of bfsm_emu.cpp, plus the gain / loss split of
// include/bfsm.h: the plans and launch sequences of bfsm_collide_split_batch_partial_async,
// bfsm_collide_bilinear_split_partial_async and bfsm_loss_rate_async (csrc/bfsm_hip.hip), run by the emulated kernel bodies.
// Built into its own shared library by tests/test_emu_split.py with the flags of tests/emu/Makefile, and into the
// stand-alone sanitizer program tests/emu/split_sanitize_main.cpp.
#include "bfsm_emu.cpp"

namespace emu {

// as for_batch() of bfsm_hip.hip: all members through every launch where the pipeline batches, else one by one
template <class Pipe, class F>
void for_batch(Pipe& p, int n_batch, F&& fn) {
    if (p.batch_together()) fn(0, n_batch);
    else for (int i = 0; i < n_batch; ++i) fn(i, 1);
}

template <class Pipe>
int collide_split_t(const bfsm_desc* d, const double* f, double* Qgain, double* nu, int n_batch, int with_loss) {
    EmuBackend be;
    Pipe p;
    std::string err;
    int rc = p.init(*d, &be, err);
    if (rc) return rc;
    if (n_batch < 1 || n_batch > p.max_batch) { p.destroy(); return BFSM_ERR_INVALID; }
    const size_t G = p.plan.G();
    double* nu_w = with_loss ? nu : nullptr;
    for_batch(p, n_batch, [&](int i0, int nb) {
        const size_t o = (size_t)i0 * G;
        const bool fu = p.fuse_reduce();
        p.gain_partial(f + o, nb, !fu);
        p.finish(Qgain + o, nullptr, with_loss != 0, nb, fu, nullptr, nu_w ? nu_w + o : nullptr);
    });
    p.destroy();
    return be.failed ? 99 : 0;
}

template <class Pipe>
int bilinear_split_t(const bfsm_desc* d, const double* g, const double* f, double* Qgain, double* nu, int with_loss) {
    EmuBackend be;
    Pipe p;
    std::string err;
    int rc = p.init(*d, &be, err);
    if (rc) return rc;
    p.collide_bilinear(Qgain, g, f, with_loss != 0, with_loss ? nu : nullptr);
    p.destroy();
    return be.failed ? 99 : 0;
}

template <class Pipe>
int loss_rate_t(const bfsm_desc* d, const double* f, double* nu, int n_batch) {
    EmuBackend be;
    Pipe p;
    std::string err;
    int rc = p.init(*d, &be, err);
    if (rc) return rc;
    if (n_batch < 1 || n_batch > p.max_batch) { p.destroy(); return BFSM_ERR_INVALID; }
    const size_t G = p.plan.G();
    for_batch(p, n_batch, [&](int i0, int nb) { p.loss_rate(nu + (size_t)i0 * G, f + (size_t)i0 * G, nb); });
    p.destroy();
    return be.failed ? 99 : 0;
}

// calls fn with the pipeline type that serves the descriptor
#define BFSM_EMU_DISPATCH(d, call)                                                                         \
    (bfsm::fused_grid(*(d))                                                                                \
         ? ((d)->precision == BFSM_F64 ? call<bfsm::Pipeline<double, emu::EmuBackend>> : call<bfsm::Pipeline<float, emu::EmuBackend>>)                 \
         : ((d)->precision == BFSM_F64 ? call<bfsm::GenericPipeline<double, emu::EmuBackend>> : call<bfsm::GenericPipeline<float, emu::EmuBackend>>))

}  // namespace emu

extern "C" {

// Emulated bfsm_collide_split_batch_partial_async on host arrays ([n_batch][G]); nu may be NULL with with_loss = 0.
int bfsm_emu_collide_split(const bfsm_desc* d, const double* f, double* Qgain, double* nu, int n_batch, int with_loss) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    if (with_loss && !nu) return BFSM_ERR_INVALID;
    return BFSM_EMU_DISPATCH(d, emu::collide_split_t)(d, f, Qgain, nu, n_batch, with_loss);
}

// Emulated bfsm_collide_bilinear_split_partial_async.
int bfsm_emu_collide_bilinear_split(const bfsm_desc* d, const double* g, const double* f, double* Qgain, double* nu, int with_loss) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    if (with_loss && !nu) return BFSM_ERR_INVALID;
    if (d->flags & BFSM_FLAG_EXACT_REDUCTIONS) return BFSM_ERR_UNSUPPORTED;
    return BFSM_EMU_DISPATCH(d, emu::bilinear_split_t)(d, g, f, Qgain, nu, with_loss);
}

// Emulated bfsm_loss_rate_async.
int bfsm_emu_loss_rate(const bfsm_desc* d, const double* f, double* nu, int n_batch) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    return BFSM_EMU_DISPATCH(d, emu::loss_rate_t)(d, f, nu, n_batch);
}

}  // extern "C"
