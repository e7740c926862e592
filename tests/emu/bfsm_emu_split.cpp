// bfsm_emu_split.cpp -- TEST HARNESS ONLY.  The host lock-step emulator of bfsm_emu.cpp, plus the gain / loss split of
// include/bfsm.h: the plans and the launch sequences bfsm_collide_split_batch_partial_async,
// bfsm_collide_bilinear_split_partial_async and bfsm_loss_rate_async call (csrc/bfsm_calls.hpp, collide_split and loss_rate;
// the pipelines' collide_bilinear), run by the emulated kernel bodies.
// Built into its own shared library by tests/test_emu_split.py with the flags of tests/emu/Makefile, and into the
// stand-alone sanitizer program tests/emu/split_sanitize_main.cpp.
#include "bfsm_emu.cpp"

extern "C" {

// Emulated bfsm_collide_split_batch_partial_async on host arrays ([n_batch][G]); nu may be NULL with with_loss = 0.
int bfsm_emu_collide_split(const bfsm_desc* d, const double* f, double* Qgain, double* nu, int n_batch, int with_loss) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    if (with_loss && !nu) return BFSM_ERR_INVALID;
    // the library's rule for the fused reduce
    return emu::with_pipeline(d, n_batch, [&](auto& p) { bfsm::collide_split(p, Qgain, nu, f, n_batch, with_loss != 0, p.fuse_reduce()); });
}

// Emulated bfsm_collide_bilinear_split_partial_async.
int bfsm_emu_collide_bilinear_split(const bfsm_desc* d, const double* g, const double* f, double* Qgain, double* nu, int with_loss) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    if (with_loss && !nu) return BFSM_ERR_INVALID;
    if (d->flags & BFSM_FLAG_EXACT_REDUCTIONS) return BFSM_ERR_UNSUPPORTED;
    return emu::with_pipeline(d, 1, [&](auto& p) { p.collide_bilinear(Qgain, g, f, with_loss != 0, with_loss ? nu : nullptr); });
}

// Emulated bfsm_loss_rate_async.
int bfsm_emu_loss_rate(const bfsm_desc* d, const double* f, double* nu, int n_batch) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    return emu::with_pipeline(d, n_batch, [&](auto& p) { bfsm::loss_rate(p, nu, f, n_batch); });
}

}  // extern "C"
