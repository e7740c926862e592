// chunks_sanitize_main.cpp -- TEST HARNESS ONLY.  Stand-alone program (no Python) that runs the fused sequence of the
// size-generic path through the host lock-step emulator on plans whose LAST chunk of directions launches more
// plane-accumulate groups than a full chunk does (csrc/bfsm_generic.hpp, groups_for is not monotone), with the loss term, in
// both precisions, single and as a batch of two on a max_batch = 2 handle, for a sanitizer build: every slab index of every
// emulated thread is checked against the allocation init made.  The plans depend on the grouping, so build it twice (from
// tests/emu):
//   g++ -O1 -g1 -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-unknown-pragmas -DBFSM_GEN_TARGET_WGS=24 \
//       -o chunks_sanitize_24 chunks_sanitize_main.cpp && ASAN_OPTIONS=detect_leaks=0 ./chunks_sanitize_24
//   ... -DBFSM_GEN_TARGET_WGS=512 -o chunks_sanitize_512 chunks_sanitize_main.cpp && ASAN_OPTIONS=detect_leaks=0 ./chunks_sanitize_512
// (the emulator's threads are ucontext coroutines on heap stacks, which the leak checker's stack scan does not follow).
// Each chunked result is also compared with the same shard in one chunk, so that a run is more than "no report".
#include <cmath>
#include <cstdio>

#include "bfsm_emu.cpp"

#ifndef BFSM_GEN_TARGET_WGS
#error "build with -DBFSM_GEN_TARGET_WGS=24 or =512: the plans below are ragged under those groupings"
#endif

struct Case { int nx, ny, nz, n_gl, n_sph; long long d0, d1; int max_chunk; };

static int run(const Case& c, int precision, int nb) {
    const size_t G = (size_t)c.nx * c.ny * c.nz;
    std::vector<double> gn(c.n_gl), gw(c.n_gl), sx(c.n_sph), sy(c.n_sph), sz(c.n_sph), sw(c.n_sph);
    for (int r = 0; r < c.n_gl; ++r) { gn[r] = 10.0 * (r + 0.5) / c.n_gl; gw[r] = 10.0 / c.n_gl * (1.0 + 0.1 * r); }
    for (int s = 0; s < c.n_sph; ++s) {       // a spiral on the sphere: no antipodal pairs, no symmetry
        const double z = 1.0 - 2.0 * (s + 0.5) / c.n_sph, rho = std::sqrt(1.0 - z * z), phi = 2.399963229728653 * s;
        sx[s] = rho * std::cos(phi); sy[s] = rho * std::sin(phi); sz[s] = z; sw[s] = 12.566370614359172 / c.n_sph * (1.0 + 0.05 * (s % 3));
    }
    bfsm_desc d{};
    d.nvx = c.nx; d.nvy = c.ny; d.nvz = c.nz; d.n_gl = c.n_gl; d.n_sph = c.n_sph;
    d.gl_nodes = gn.data(); d.gl_wts = gw.data(); d.sph_wts = sw.data(); d.sx = sx.data(); d.sy = sy.data(); d.sz = sz.data();
    d.gamma = 0.5; d.b_gamma = 0.3; d.L = 11.0; d.precision = precision; d.max_batch = nb > 1 ? nb : 0;
    d.dir_begin = c.d0; d.dir_end = c.d1;
    std::vector<double> f(nb * G), Q(nb * G), Q1(nb * G);
    unsigned long long st = 88172645463325252ull;
    for (double& v : f) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; v = 0.1 + (double)(st >> 11) / 9007199254740992.0; }
    std::printf("%d x %d x %d fp%d, directions [%lld, %lld) of %d x %d, max_chunk %d, batch %d: ", c.nx, c.ny, c.nz, precision, c.d0,
                c.d1, c.n_gl, c.n_sph, c.max_chunk, nb);
    std::fflush(stdout);
    d.max_chunk = c.max_chunk;
    int rc = bfsm_emu_collide_batch(&d, f.data(), Q.data(), nullptr, nb);      // gain of the shard + the loss term
    if (rc) { std::printf("rc=%d\n", rc); return 1; }
    d.max_chunk = 0;                                                         // the same shard in one chunk
    rc = bfsm_emu_collide_batch(&d, f.data(), Q1.data(), nullptr, nb);
    if (rc) { std::printf("one-chunk rc=%d\n", rc); return 1; }
    double e = 0, qmax = 0;
    for (size_t i = 0; i < nb * G; ++i) { e = std::fmax(e, std::fabs(Q[i] - Q1[i])); qmax = std::fmax(qmax, std::fabs(Q1[i])); }
    const double tol = precision == 64 ? 1e-12 : 2e-5;
    std::printf("|Q - Q(one chunk)| / max|Q| = %.2e\n", e / qmax);
    return e <= tol * qmax ? 0 : 1;
}

int main() {
#if BFSM_GEN_TARGET_WGS == 24
    const Case cases[] = {{8, 4, 12, 3, 12, 0, 7, 4}};                      // plane-accumulate groups 2, then 3
#else
    const Case cases[] = {{32, 8, 8, 6, 6, 0, 33, 17},                      // groups 9, then 16
                          {16, 8, 6, 6, 12, 0, 0, 40}};                     // groups 20, then 32
#endif
    int bad = 0;
    for (const Case& c : cases)
        for (int precision : {64, 32})
            for (int nb : {1, 2}) bad += run(c, precision, nb);
    std::printf(bad ? "FAILED\n" : "chunks sanitizer run (grouping %d): clean\n", BFSM_GEN_TARGET_WGS);
    return bad ? 1 : 0;
}
