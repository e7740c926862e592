// TEST ONLY (GPU).  The batched two-operand calls of BoltzmannOperator<HIP_Backend> (the C++ mirror of
// bfsm_collide_symmetric_batch, bfsm_collide_symmetric_batch_partial_async and bfsm_collide_bilinear_batch_partial_async) at N = 24
// with the shipped 12-point design: on an exact + Hermitian handle of max_batch 3, computeSymmetricCollisionBatch with a shared f
// and without sharing, every member bit for bit the same handle's computeSymmetricCollision; collideSymmetricBatchPartial on a
// stream the same bits; on a faithful handle collideBilinearBatchPartial with a shared g against bfsm_collide_bilinear.  Built and
// run by tests/test_gpu_symmetric_batch.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "Collisions/HIPBoltzmannOperator.hpp"
#include "Utilities/constants.hpp"

#define OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)
static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

int main(int argc, char** argv) {
    if (argc > 1) SphericalDesign::setDataDirectory(argv[1]);
    const int Nv = 24, Ngl = 2, Ns = 12, NB = 3;
    const size_t G = (size_t)Nv * Nv * Nv;
    const double gamma = 0, b_gamma = 1 / (4 * pi), S = 5, R = 3, L = ((3 + std::sqrt(2.0)) / 2) * S;
    std::vector<double> f_h(NB * G), g_h(NB * G);
    unsigned long long lcg = 12345;
    auto draw = [&]() { lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(lcg >> 11) / 9007199254740992.0 - 0.45; };
    for (double& v : f_h) v = draw();
    for (double& v : g_h) v = draw();

    OK(hipSetDevice(0));
    double *f_d, *g_d, *q_d, *q1_d;
    OK(hipMalloc((void**)&f_d, NB * G * sizeof(double)));
    OK(hipMalloc((void**)&g_d, NB * G * sizeof(double)));
    OK(hipMalloc((void**)&q_d, NB * G * sizeof(double)));
    OK(hipMalloc((void**)&q1_d, G * sizeof(double)));
    OK(hipMemcpy(f_d, f_h.data(), NB * G * sizeof(double), hipMemcpyHostToDevice));
    OK(hipMemcpy(g_d, g_h.data(), NB * G * sizeof(double), hipMemcpyHostToDevice));
    hipStream_t stream;
    OK(hipStreamCreate(&stream));

    auto gl = std::make_shared<GaussLegendreQuadrature>(Ngl, 0, R);
    auto sph = std::make_shared<SphericalDesign>(Ns);
    std::vector<double> q(NB * G), q1(G);
    double qmax = 0;
    for (int faithful = 0; faithful < 2; ++faithful) {
        BoltzmannOperator<HIP_Backend> op(gl, sph, Nv, Nv, Nv, gamma, b_gamma, L);
        if (!faithful) op.setExactReductions(true, true);
        op.setMaxBatch(NB);
        op.initialize();
        for (int share : {(int)BFSM_SHARE_NONE, (int)BFSM_SHARE_F, (int)BFSM_SHARE_G})
            for (int form = 0; form < (faithful ? 3 : 2); ++form) {       // 0: blocking symmetric, 1: partial on a stream, 2: bilinear
                OK(hipMemset(q_d, 0xFF, NB * G * sizeof(double)));
                if (form == 0) op.computeSymmetricCollisionBatch(q_d, g_d, f_d, NB, share);
                else if (form == 1) op.collideSymmetricBatchPartial(q_d, g_d, f_d, NB, share, true, stream);
                else op.collideBilinearBatchPartial(q_d, g_d, f_d, NB, share, true, stream);
                OK(hipStreamSynchronize(stream));
                OK(hipMemcpy(q.data(), q_d, NB * G * sizeof(double), hipMemcpyDeviceToHost));
                for (int i = 0; i < NB; ++i) {
                    const double* gi = g_d + (share == BFSM_SHARE_G ? 0 : i * G);
                    const double* fi = f_d + (share == BFSM_SHARE_F ? 0 : i * G);
                    if (form < 2) op.computeSymmetricCollision(q1_d, gi, fi);
                    else CHECK(bfsm_collide_bilinear(op.handle(), q1_d, gi, fi) == BFSM_OK);
                    OK(hipMemcpy(q1.data(), q1_d, G * sizeof(double), hipMemcpyDeviceToHost));
                    CHECK(std::memcmp(q1.data(), q.data() + i * G, G * sizeof(double)) == 0);
                    for (double v : q1) qmax = std::fmax(qmax, std::fabs(v));
                }
            }
        if (!faithful) CHECK(bfsm_collide_bilinear_batch_partial_async(op.handle(), q_d, g_d, f_d, NB, BFSM_SHARE_NONE, 1, nullptr) == BFSM_ERR_UNSUPPORTED);
    }
    CHECK(qmax > 0 && std::isfinite(qmax));
    std::printf("every batch member equals the single call bit for bit (max |Q| %.3g)\n", qmax);

    OK(hipStreamDestroy(stream));
    OK(hipFree(f_d));
    OK(hipFree(g_d));
    OK(hipFree(q_d));
    OK(hipFree(q1_d));
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("symmetric batch mirror checks passed\n");
    return 0;
}
