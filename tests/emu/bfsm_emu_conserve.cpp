// bfsm_emu_conserve.cpp -- TEST HARNESS ONLY.  The host lock-step emulator of bfsm_emu.cpp, plus the conservative projection
// of csrc/bfsm_conserve.hpp: the same Conserver host code and kernel bodies as BFSM_FLAG_CONSERVE / bfsm_conserve_async, run
// on host arrays.  Built into its own shared library by tests/test_emu_conserve.py with the flags of tests/emu/Makefile.
#include "bfsm_emu.cpp"
#include "../../boltzmann-fourier-spectral-method_amd/csrc/bfsm_conserve.hpp"

namespace emu {

// EmuBackend plus the launcher of the projection kernels (bfsm_hip.hip: HipBackend::launch_cons)
struct ConsEmuBackend : EmuBackend {
    template <bfsm::CK kind>
    static void body_cons(void* a, EmuCtx& ctx) {
        using namespace bfsm;
        const ConsParams& prm = *static_cast<const ConsParams*>(a);
        BFSM_RUN_CONS_BODY(kind, prm, ctx)
    }
    template <bfsm::CK kind>
    void launch_cons(int gx, int gy, const bfsm::ConsParams& prm) {
        smem.assign(bfsm::CONS_LDS_BYTES, 0xCD);
        bfsm::ConsParams copy = prm;
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx) {
                sched.run_block(bfsm::CONS_THREADS, bx, by, 0, smem.data(), &body_cons<kind>, &copy, gx, gy);
                if (sched.deadlock) failed = true;
            }
    }
};

}  // namespace emu

extern "C" {

// Emulated bfsm_conserve_async on host arrays: Q (n_batch * G doubles) := PQ in place.  form: -1 the library's choice,
// 0 the two-launch form (moments + apply), 1 the one-launch form.  info (optional, 2 ints): W, the form used.
int bfsm_emu_conserve(const bfsm_desc* d, double* Q, int n_batch, int form, int* info) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    emu::ConsEmuBackend be;
    bfsm::Conserver<emu::ConsEmuBackend> c;
    rc = c.init(*d, &be, err);
    if (rc) return rc;
    if (n_batch < 1 || n_batch > c.max_batch) { c.destroy(); return BFSM_ERR_INVALID; }
    if (form >= 0) c.small = form == 1;
    if (info) { info[0] = c.prm.W; info[1] = c.small ? 1 : 0; }
    c.apply(Q, n_batch);
    c.destroy();
    return be.failed ? 99 : 0;
}

}  // extern "C"
