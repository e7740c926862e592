// TEST ONLY (GPU).  BoltzmannOperator<HIP_Backend>::moments / maxwellian (the C++ mirror of bfsm_moments_async /
// bfsm_maxwellian_async) on the BKW state at N = 16, against host loops at the tolerances of tests/moments_ref.py: each of the
// six grid sums within 64 eps dV sum |psi_k f|, u and T within 1e-13 of their scales, the Maxwellian within 64 eps max M of
// the host formula evaluated from the row the device produced.  Built and run by tests/test_gpu_moments.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
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
    const int Nv = 16, Ngl = 2, Ns = 6;
    const size_t G = (size_t)Nv * Nv * Nv;
    const double gamma = 0, b_gamma = 1 / (4 * pi), S = 5, R = 2 * S, L = ((3 + std::sqrt(2.0)) / 2) * S;
    const double dv = 2 * L / Nv, dV = dv * dv * dv, t = 6.5, K = 1 - std::exp(-t / 6);
    std::vector<double> v(Nv), f_h(G);
    for (int i = 0; i < Nv; ++i) v[i] = -L + (i + 0.5) * dv;
    for (int i = 0; i < Nv; ++i)
        for (int j = 0; j < Nv; ++j)
            for (int k = 0; k < Nv; ++k) {
                const double r2 = v[i] * v[i] + v[j] * v[j] + v[k] * v[k];
                f_h[((size_t)i * Nv + j) * Nv + k] =
                    std::exp(-r2 / (2 * K)) * ((5 * K - 3) / K + (1 - K) / (K * K) * r2) / (2 * std::pow(2 * pi * K, 1.5));
            }

    // host sums (long double) and their scales
    long double s[6] = {0, 0, 0, 0, 0, 0}, a[6] = {0, 0, 0, 0, 0, 0}, av[3] = {0, 0, 0};
    for (int i = 0; i < Nv; ++i)
        for (int j = 0; j < Nv; ++j)
            for (int k = 0; k < Nv; ++k) {
                const long double f = f_h[((size_t)i * Nv + j) * Nv + k];
                const long double c[3] = {v[i], v[j], v[k]};
                const long double term[6] = {f, c[0] * f, c[1] * f, c[2] * f, (c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) * f,
                                             f > 0 ? f * std::log(f) : 0.0L};
                for (int m = 0; m < 6; ++m) { s[m] += term[m]; a[m] += std::fabs(term[m]); }
                for (int m = 0; m < 3; ++m) av[m] += std::fabs(c[m] * f);
            }
    for (int m = 0; m < 6; ++m) { s[m] *= dV; a[m] *= dV; }

    OK(hipSetDevice(0));
    double *f_d, *mom_d, *M_d;
    OK(hipMalloc((void**)&f_d, G * sizeof(double)));
    OK(hipMalloc((void**)&M_d, G * sizeof(double)));
    OK(hipMalloc((void**)&mom_d, BFSM_MOM_COUNT * sizeof(double)));
    OK(hipMemcpy(f_d, f_h.data(), G * sizeof(double), hipMemcpyHostToDevice));

    auto gl = std::make_shared<GaussLegendreQuadrature>(Ngl, 0, R);
    auto sph = std::make_shared<SphericalDesign>(Ns);
    BoltzmannOperator<HIP_Backend> op(gl, sph, Nv, Nv, Nv, gamma, b_gamma, L);
    op.initialize();
    op.moments(mom_d, f_d);
    op.maxwellian(M_d, mom_d);
    op.synchronize();
    double row[BFSM_MOM_COUNT];
    std::vector<double> M_h(G), f_back(G);
    OK(hipMemcpy(row, mom_d, sizeof(row), hipMemcpyDeviceToHost));
    OK(hipMemcpy(M_h.data(), M_d, G * sizeof(double), hipMemcpyDeviceToHost));
    OK(hipMemcpy(f_back.data(), f_d, G * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(f_back == f_h);

    const int col[6] = {BFSM_MOM_RHO, BFSM_MOM_MX, BFSM_MOM_MY, BFSM_MOM_MZ, BFSM_MOM_E, BFSM_MOM_H};
    for (int m = 0; m < 6; ++m) {
        const double err = (double)std::fabs((long double)row[col[m]] - s[m]), tol = 64 * DBL_EPSILON * (double)a[m];
        std::printf("sum %d: device %.17g host %.17Lg error %.3g tolerance %.3g\n", m, row[col[m]], s[m], err, tol);
        CHECK(err <= tol);
    }
    const long double rho = s[0], u[3] = {s[1] / rho, s[2] / rho, s[3] / rho};
    const long double T = (s[4] / rho - (u[0] * u[0] + u[1] * u[1] + u[2] * u[2])) / 3;
    for (int m = 0; m < 3; ++m) {
        const double err = (double)std::fabs((long double)row[BFSM_MOM_UX + m] - u[m]), tol = 1e-13 * (double)(dV * av[m] / rho);
        std::printf("u %d: error %.3g tolerance %.3g\n", m, err, tol);
        CHECK(err <= tol);
    }
    {
        const double err = (double)std::fabs((long double)row[BFSM_MOM_T] - T), tol = 1e-13 * (double)(a[4] / rho);
        std::printf("T: device %.17g error %.3g tolerance %.3g\n", row[BFSM_MOM_T], err, tol);
        CHECK(err <= tol);
    }
    CHECK(std::fabs(row[BFSM_MOM_RHO] - 1.0) < 0.1 && std::fabs(row[BFSM_MOM_T] - 1.0) < 0.1);   // BKW: rho = T = 1, coarsely resolved at N = 16

    double merr = 0, mmax = 0;
    const double coef = row[BFSM_MOM_RHO] / std::pow(2 * pi * row[BFSM_MOM_T], 1.5);
    for (int i = 0; i < Nv; ++i)
        for (int j = 0; j < Nv; ++j)
            for (int k = 0; k < Nv; ++k) {
                const double cx = v[i] - row[BFSM_MOM_UX], cy = v[j] - row[BFSM_MOM_UY], cz = v[k] - row[BFSM_MOM_UZ];
                const double want = coef * std::exp(-(cx * cx + cy * cy + cz * cz) / (2 * row[BFSM_MOM_T]));
                merr = std::max(merr, std::fabs(M_h[((size_t)i * Nv + j) * Nv + k] - want));
                mmax = std::max(mmax, want);
            }
    std::printf("Maxwellian: error %.3g tolerance %.3g\n", merr, 64 * DBL_EPSILON * mmax);
    CHECK(merr <= 64 * DBL_EPSILON * mmax);

    OK(hipFree(f_d));
    OK(hipFree(M_d));
    OK(hipFree(mom_d));
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("moments mirror checks passed\n");
    return 0;
}
