// bfsm_emu_symmetric.cpp -- TEST HARNESS ONLY.  The host lock-step emulator of bfsm_emu.cpp, plus the symmetric form
// Qs(g,f) = Q(g,f) + Q(f,g): the same plan and launch sequence as bfsm_collide_symmetric_partial_async (bfsm_calls.hpp,
// collide_symmetric: Pipeline::collide_symmetric on the fused cubes in every mode, GenericPipeline::collide_symmetric on every
// other box), run by the emulated kernel bodies.  Built into its own shared library by tests/test_emu_symmetric.py with the
// flags of tests/emu/Makefile.
#include "bfsm_emu.cpp"

extern "C" {

// Emulated bfsm_collide_symmetric_partial_async (with_loss = 1 and all directions: bfsm_collide_symmetric) on host arrays.
int bfsm_emu_collide_symmetric(const bfsm_desc* d, const double* g, const double* f, double* Q, int with_loss) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    return emu::with_pipeline(d, 1, [&](auto& p) { bfsm::collide_symmetric(p, Q, g, f, with_loss != 0); });
}

// What make_plan decides for a descriptor: info[0..5] = antipodal, sph_eff, weight_mult, hermitian, chunks, slabs
int bfsm_emu_symmetric_plan(const bfsm_desc* d, int* info) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    if (!bfsm::fused_grid(*d)) return BFSM_ERR_UNSUPPORTED;
    const bfsm::PlanInfo p = bfsm::make_plan(*d);
    info[0] = p.antipodal ? 1 : 0; info[1] = p.sph_eff; info[2] = p.weight_mult; info[3] = p.hermitian ? 1 : 0;
    info[4] = (int)p.chunks.size(); info[5] = (int)p.segs.size();
    return BFSM_OK;
}

}  // extern "C"
