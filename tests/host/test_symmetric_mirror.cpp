// TEST ONLY (GPU).  BoltzmannOperator<HIP_Backend>::computeSymmetricCollision (the C++ mirror of bfsm_collide_symmetric) on an
// exact + Hermitian handle at N = 24 with the shipped 12-point design (antipodal: merged to 6 directions), against the same
// handle's computeCollision, which the suite pins to the oracle: Qs(f,f) = 2 Q(f,f) and the polarization identity
// Qs(g,f) = Q(f+g) - Q(f) - Q(g), both within 1e-12 of max|Qs|; g is sign-indefinite and has no symmetry.  The bilinear
// overload still reports BFSM_ERR_UNSUPPORTED on that handle.  Built and run by tests/test_gpu_symmetric.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "Collisions/HIPBoltzmannOperator.hpp"
#include "Utilities/constants.hpp"

#define OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)
static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

int main(int argc, char** argv) {
    if (argc > 1) SphericalDesign::setDataDirectory(argv[1]);
    const int Nv = 24, Ngl = 2, Ns = 12;
    const size_t G = (size_t)Nv * Nv * Nv;
    const double gamma = 0, b_gamma = 1 / (4 * pi), S = 5, R = 3, L = ((3 + std::sqrt(2.0)) / 2) * S;
    const double dv = 2 * L / Nv;
    std::vector<double> f_h(G), g_h(G), s_h(G);
    unsigned long long lcg = 12345;
    for (int i = 0; i < Nv; ++i)
        for (int j = 0; j < Nv; ++j)
            for (int k = 0; k < Nv; ++k) {
                const double x = -L + (i + 0.5) * dv, y = -L + (j + 0.5) * dv, z = -L + (k + 0.5) * dv;
                const size_t o = ((size_t)i * Nv + j) * Nv + k;
                f_h[o] = std::exp(-((x - 0.7) * (x - 0.7) + y * y + (z + 0.4) * (z + 0.4)) / 2);
                lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
                g_h[o] = f_h[o] * ((double)(lcg >> 11) / 9007199254740992.0 - 0.45);
                s_h[o] = f_h[o] + g_h[o];
            }

    OK(hipSetDevice(0));
    double *f_d, *g_d, *s_d, *q_d;
    OK(hipMalloc((void**)&f_d, G * sizeof(double)));
    OK(hipMalloc((void**)&g_d, G * sizeof(double)));
    OK(hipMalloc((void**)&s_d, G * sizeof(double)));
    OK(hipMalloc((void**)&q_d, G * sizeof(double)));
    OK(hipMemcpy(f_d, f_h.data(), G * sizeof(double), hipMemcpyHostToDevice));
    OK(hipMemcpy(g_d, g_h.data(), G * sizeof(double), hipMemcpyHostToDevice));
    OK(hipMemcpy(s_d, s_h.data(), G * sizeof(double), hipMemcpyHostToDevice));

    auto gl = std::make_shared<GaussLegendreQuadrature>(Ngl, 0, R);
    auto sph = std::make_shared<SphericalDesign>(Ns);
    BoltzmannOperator<HIP_Backend> op(gl, sph, Nv, Nv, Nv, gamma, b_gamma, L);
    op.setExactReductions(true, true);
    op.initialize();
    CHECK(op.counters().antipodal_merged == 1);

    auto run = [&](bool symmetric, const double* a, const double* b, std::vector<double>& out) {
        if (symmetric) op.computeSymmetricCollision(q_d, a, b); else op.computeCollision(q_d, a);
        return hipMemcpy(out.data(), q_d, G * sizeof(double), hipMemcpyDeviceToHost);
    };
    std::vector<double> qff(G), qf(G), qg(G), qs(G), qgf(G);
    OK(run(true, f_d, f_d, qff));
    OK(run(false, f_d, nullptr, qf));
    OK(run(false, g_d, nullptr, qg));
    OK(run(false, s_d, nullptr, qs));
    OK(run(true, g_d, f_d, qgf));

    double e1 = 0, m1 = 0, e2 = 0, m2 = 0;
    for (size_t o = 0; o < G; ++o) {
        e1 = std::max(e1, std::fabs(qff[o] - 2 * qf[o]));
        m1 = std::max(m1, std::fabs(2 * qf[o]));
        e2 = std::max(e2, std::fabs(qgf[o] - (qs[o] - qf[o] - qg[o])));
        m2 = std::max(m2, std::fabs(qgf[o]));
    }
    std::printf("Qs(f,f) against 2 Q(f,f): max error %.3g of %.3g\n", e1, m1);
    std::printf("Qs(g,f) against Q(f+g) - Q(f) - Q(g): max error %.3g of %.3g\n", e2, m2);
    CHECK(m1 > 0 && e1 <= 1e-12 * m1);
    CHECK(m2 > 0 && e2 <= 1e-12 * m2);
    CHECK(bfsm_collide_bilinear(op.handle(), q_d, g_d, f_d) == BFSM_ERR_UNSUPPORTED);

    OK(hipFree(f_d));
    OK(hipFree(g_d));
    OK(hipFree(s_d));
    OK(hipFree(q_d));
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("symmetric mirror checks passed\n");
    return 0;
}
