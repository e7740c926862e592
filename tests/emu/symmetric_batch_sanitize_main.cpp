// symmetric_batch_sanitize_main.cpp -- TEST HARNESS ONLY.  Stand-alone program (no Python) that runs the batched symmetric and
// bilinear sequences (bfsm_calls.hpp, collide_pairs) through the host lock-step emulator for a sanitizer build: every spectrum,
// slab, segment-sum and tail index of every emulated thread is checked against the allocations Pipeline::init made for
// max_batch members.  N = 16 in the three modes and both precisions, N = 24 Hermitian; max_batch 3 with n_batch 3 and 2; every
// share mode; chunks of 2; the shard whose 2 x slabs <= 8 take the reduce fused into the tail.  From tests/emu:
//   g++ -O1 -g1 -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-unknown-pragmas -DBFSM_FUSED_N_MAX=24 \
//       -o symmetric_batch_sanitize symmetric_batch_sanitize_main.cpp && ASAN_OPTIONS=detect_leaks=0 ./symmetric_batch_sanitize
// (the emulator's threads are ucontext coroutines on heap stacks, which the leak checker's stack scan does not follow).
// Every member is also compared bit for bit with the single call on a handle of the same descriptor, so that a run is more than
// "no report".
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bfsm_emu_symmetric_batch.cpp"

struct Case { int n, precision, flags, n_gl, n_half, max_chunk; long long d0, d1; };

static int run(const Case& c, int nb, int share, int symmetric) {
    const size_t G = (size_t)c.n * c.n * c.n;
    const int n_sph = 2 * c.n_half;
    std::vector<double> gn(c.n_gl), gw(c.n_gl), sx(n_sph), sy(n_sph), sz(n_sph), sw(n_sph);
    for (int r = 0; r < c.n_gl; ++r) { gn[r] = 10.0 * (r + 0.5) / c.n_gl; gw[r] = 10.0 / c.n_gl * (1.0 + 0.1 * r); }
    for (int s = 0; s < c.n_half; ++s) {       // half a spiral and its bit-exact negation, equal weights: the exact modes merge it
        const double z = 1.0 - (s + 0.5) / c.n_half, rho = std::sqrt(1.0 - z * z), phi = 2.399963229728653 * s;
        sx[s] = rho * std::cos(phi); sy[s] = rho * std::sin(phi); sz[s] = z; sw[s] = 12.566370614359172 / n_sph * (1.0 + 0.05 * (s % 3));
        sx[s + c.n_half] = -sx[s]; sy[s + c.n_half] = -sy[s]; sz[s + c.n_half] = -sz[s]; sw[s + c.n_half] = sw[s];
    }
    bfsm_desc d{};
    d.nvx = d.nvy = d.nvz = c.n; d.n_gl = c.n_gl; d.n_sph = n_sph;
    d.gl_nodes = gn.data(); d.gl_wts = gw.data(); d.sph_wts = sw.data(); d.sx = sx.data(); d.sy = sy.data(); d.sz = sz.data();
    d.gamma = 0.5; d.b_gamma = 0.3; d.L = 11.0; d.precision = c.precision; d.max_batch = 3; d.flags = c.flags;
    d.dir_begin = c.d0; d.dir_end = c.d1; d.max_chunk = c.max_chunk;
    const size_t ng = share == BFSM_SHARE_G ? 1 : nb, nf = share == BFSM_SHARE_F ? 1 : nb;
    // exactly sized host arrays: a member stride applied to a shared operand reads past its end
    std::vector<double> g(ng * G), f(nf * G), Q(nb * G), Q1(G);
    unsigned long long st = 88172645463325252ull;
    auto draw = [&](std::vector<double>& a) { for (double& v : a) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; v = (double)(st >> 11) / 9007199254740992.0 - 0.45; } };
    draw(g); draw(f);
    std::printf("N=%d fp%d flags %d, directions [%lld, %lld) of %d x %d, max_chunk %d, %s, n_batch %d, share %d: ", c.n, c.precision,
                c.flags, c.d0, c.d1, c.n_gl, n_sph, c.max_chunk, symmetric ? "symmetric" : "bilinear", nb, share);
    std::fflush(stdout);
    int rc = bfsm_emu_collide_pairs(&d, g.data(), f.data(), Q.data(), nb, share, 1, symmetric, nullptr);
    if (rc) { std::printf("rc=%d\n", rc); return 1; }
    int diff = 0;
    for (int i = 0; i < nb; ++i) {
        rc = bfsm_emu_collide_pair_single(&d, g.data() + (ng > 1 ? i * G : 0), f.data() + (nf > 1 ? i * G : 0), Q1.data(), 1, symmetric, nullptr);
        if (rc) { std::printf("single rc=%d\n", rc); return 1; }
        if (std::memcmp(Q1.data(), Q.data() + i * G, G * sizeof(double)) != 0) ++diff;
    }
    std::printf("%d of %d members differ from the single call\n", diff, nb);
    return diff ? 1 : 0;
}

int main() {
    const int EX = BFSM_FLAG_EXACT_REDUCTIONS, HE = BFSM_FLAG_EXACT_REDUCTIONS | BFSM_FLAG_HERMITIAN;
    int bad = 0;
    for (int precision : {64, 32})
        for (int flags : {0, EX, HE}) {
            const Case c{16, precision, flags, 2, 3, 0, 0, 0};
            bad += run(c, 3, BFSM_SHARE_NONE, 1) + run(c, 2, BFSM_SHARE_G, 1) + run(c, 3, BFSM_SHARE_F, 1);
            if (!flags) bad += run(c, 3, BFSM_SHARE_G, 0) + run(c, 2, BFSM_SHARE_F, 0);
        }
    const Case herm24{24, 64, HE, 2, 3, 0, 0, 0}, chunks{24, 64, HE, 3, 3, 2, 0, 0}, shard{24, 64, HE, 2, 3, 0, 0, 6};
    bad += run(herm24, 3, BFSM_SHARE_F, 1);
    bad += run(chunks, 2, BFSM_SHARE_G, 1);
    bad += run(shard, 2, BFSM_SHARE_NONE, 1) + run(shard, 3, BFSM_SHARE_F, 1);
    std::printf(bad ? "FAILED\n" : "symmetric batch sanitizer run: clean\n");
    return bad ? 1 : 0;
}
