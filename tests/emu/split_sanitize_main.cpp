// split_sanitize_main.cpp -- TEST HARNESS ONLY.  Stand-alone program (no Python) that runs the gain / loss split and the
// loss-only sequence through the host lock-step emulator at 16^3 (fused pipeline) and 12 x 8 x 20 (size-generic path), both
// precisions, for a sanitizer build: every LDS / global index of every emulated thread is checked against the allocation the
// launch would make.  Build and run (from tests/emu):
//   g++ -O1 -g1 -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-unknown-pragmas -DBFSM_GEN_TARGET_WGS=24 \
//       -o split_sanitize split_sanitize_main.cpp && ASAN_OPTIONS=detect_leaks=0 ./split_sanitize
// (the emulator's threads are ucontext coroutines on heap stacks, which the leak checker's stack scan does not follow).
// Also checks the identity Q = Qgain - f nu against the emulated combined call, so that a run is more than "no report".
#include <cmath>
#include <cstdio>

#include "bfsm_emu_split.cpp"

static int run(int nx, int ny, int nz, int precision) {
    const size_t G = (size_t)nx * ny * nz;
    const int nb = 2;
    const double gl_nodes[2] = {2.5, 7.0}, gl_wts[2] = {3.0, 2.0};
    const double s = 1.0 / std::sqrt(3.0);
    const double sx[3] = {1.0, 0.0, s}, sy[3] = {0.0, 0.6, s}, sz[3] = {0.0, 0.8, -s}, sw[3] = {4.0, 5.0, 3.5};
    bfsm_desc d{};
    d.nvx = nx; d.nvy = ny; d.nvz = nz; d.n_gl = 2; d.n_sph = 3;
    d.gl_nodes = gl_nodes; d.gl_wts = gl_wts; d.sph_wts = sw; d.sx = sx; d.sy = sy; d.sz = sz;
    d.gamma = 0.5; d.b_gamma = 0.3; d.L = 11.0; d.precision = precision; d.max_batch = nb;
    std::vector<double> f(nb * G), Qg(nb * G), nu(nb * G), nu1(nb * G), Q(nb * G);
    unsigned long long st = 88172645463325252ull;
    for (double& v : f) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; v = 0.1 + (double)(st >> 11) / 9007199254740992.0; }
    int rc = bfsm_emu_collide_split(&d, f.data(), Qg.data(), nu.data(), nb, 1);
    if (rc) { std::printf("split rc=%d\n", rc); return 1; }
    rc = bfsm_emu_loss_rate(&d, f.data(), nu1.data(), nb);
    if (rc) { std::printf("loss_rate rc=%d\n", rc); return 1; }
    rc = bfsm_emu_collide_batch(&d, f.data(), Q.data(), nullptr, nb);
    if (rc) { std::printf("collide rc=%d\n", rc); return 1; }
    double e_id = 0, e_nu = 0, qmax = 0, numax = 0;
    for (size_t i = 0; i < nb * G; ++i) {
        e_id = std::fmax(e_id, std::fabs(Qg[i] - f[i] * nu[i] - Q[i]));
        e_nu = std::fmax(e_nu, std::fabs(nu[i] - nu1[i]));
        qmax = std::fmax(qmax, std::fabs(Q[i]));
        numax = std::fmax(numax, std::fabs(nu[i]));
    }
    const double tol = precision == 64 ? 1e-12 : 5e-6;
    std::printf("%d x %d x %d fp%d: |Qgain - f nu - Q| / max|Q| = %.2e, |nu - loss-only nu| / max|nu| = %.2e\n", nx, ny, nz, precision,
                e_id / qmax, e_nu / numax);
    return (e_id <= tol * qmax && e_nu <= tol * numax) ? 0 : 1;
}

int main() {
    int bad = 0;
    for (int precision : {64, 32}) {
        bad += run(16, 16, 16, precision);
        bad += run(12, 8, 20, precision);
    }
    std::printf(bad ? "FAILED\n" : "split sanitizer run: clean\n");
    return bad ? 1 : 0;
}
