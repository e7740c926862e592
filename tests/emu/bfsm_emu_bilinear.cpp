// bfsm_emu_bilinear.cpp -- TEST HARNESS ONLY.  The host lock-step emulator of bfsm_emu.cpp, plus the bilinear form Q(g,f):
// the same plan and launch sequence as bfsm_collide_bilinear_partial_async (Pipeline::collide_bilinear on the fused cubes,
// GenericPipeline::collide_bilinear on every other box), run by the emulated kernel bodies.  Built into its own shared
// library by tests/test_emu_bilinear.py with the flags of tests/emu/Makefile.
#include "bfsm_emu.cpp"

extern "C" {

// Emulated bfsm_collide_bilinear_partial_async (with_loss = 1 and all directions: bfsm_collide_bilinear) on host arrays.
int bfsm_emu_collide_bilinear(const bfsm_desc* d, const double* g, const double* f, double* Q, int with_loss) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    if (d->flags & BFSM_FLAG_EXACT_REDUCTIONS) return BFSM_ERR_UNSUPPORTED;
    return emu::with_pipeline(d, 1, [&](auto& p) { p.collide_bilinear(Q, g, f, with_loss != 0); });
}

}  // extern "C"
