// bfsm_emu_moments.cpp -- TEST HARNESS ONLY.  The host lock-step emulator of bfsm_emu.cpp, plus the moments / Maxwellian module
// of csrc/bfsm_moments.hpp: the same Macroscopic host code and kernel bodies as bfsm_moments_async / bfsm_maxwellian_async, run
// on host arrays.  Built into its own shared library by tests/test_emu_moments.py with the flags of tests/emu/Makefile.
#include "bfsm_emu.cpp"
#include "../../boltzmann-fourier-spectral-method_amd/csrc/bfsm_moments.hpp"

namespace emu {

// EmuBackend plus the launcher of the moment kernels (bfsm_hip.hip: HipBackend::launch_mom)
struct MomEmuBackend : EmuBackend {
    template <bfsm::MK kind>
    static void body_mom(void* a, EmuCtx& ctx) {
        using namespace bfsm;
        const MomParams& prm = *static_cast<const MomParams*>(a);
        BFSM_RUN_MOM_BODY(kind, prm, ctx)
    }
    template <bfsm::MK kind>
    void launch_mom(int gx, int gy, const bfsm::MomParams& prm) {
        smem.assign(bfsm::MOM_LDS_BYTES, 0xCD);
        bfsm::MomParams copy = prm;
        for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx) {
                sched.run_block(bfsm::MOM_THREADS, bx, by, 0, smem.data(), &body_mom<kind>, &copy, gx, gy);
                if (sched.deadlock) failed = true;
            }
    }
};

static int with_macro(const bfsm_desc* d, int n_batch, int form, int* info, void (*run)(bfsm::Macroscopic<MomEmuBackend>&, void*),
                      void* arg) {
    std::string err;
    int rc = bfsm::validate_desc(*d, err);
    if (rc) return rc;
    MomEmuBackend be;
    bfsm::Macroscopic<MomEmuBackend> m;
    rc = m.init(*d, &be, err);
    if (rc) return rc;
    if (n_batch < 1 || n_batch > m.max_batch) { m.destroy(); return BFSM_ERR_INVALID; }
    if (info) { info[0] = m.prm.W; info[1] = m.small ? 1 : 0; }      // what init chose
    if (form >= 0) m.small = form == 1;
    run(m, arg);
    m.destroy();
    return be.failed ? 99 : 0;
}

}  // namespace emu

extern "C" {

// Emulated bfsm_moments_async on host arrays: mom (n_batch * BFSM_MOM_COUNT doubles) from f (n_batch * G doubles).  form: -1
// the library's choice, 0 Sums + Finish, 1 Small.  info (optional, 2 ints): W and the form init chose.
int bfsm_emu_moments(const bfsm_desc* d, const double* f, double* mom, int n_batch, int form, int* info) {
    struct A { const double* f; double* mom; int nb; } a{f, mom, n_batch};
    return emu::with_macro(d, n_batch, form, info, [](bfsm::Macroscopic<emu::MomEmuBackend>& m, void* p) {
        A& x = *static_cast<A*>(p);
        m.moments(x.mom, x.f, x.nb);
    }, &a);
}

// Emulated bfsm_maxwellian_async on host arrays: M (n_batch * G doubles) from mom (n_batch rows).
int bfsm_emu_maxwellian(const bfsm_desc* d, const double* mom, double* M, int n_batch) {
    struct A { const double* mom; double* M; int nb; } a{mom, M, n_batch};
    return emu::with_macro(d, n_batch, -1, nullptr, [](bfsm::Macroscopic<emu::MomEmuBackend>& m, void* p) {
        A& x = *static_cast<A*>(p);
        m.maxwellian(x.M, x.mom, x.nb);
    }, &a);
}

}  // extern "C"
