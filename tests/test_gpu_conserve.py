"""-m gpu: the conservative projection (include/bfsm.h: BFSM_FLAG_CONSERVE, bfsm_conserve_async) on the MI355X.

On every kernel route: the moments of PQ vanish to fp64 rounding, the flagged output is the numpy projection
(tests/conserve_ref.py) of the unflagged output, and it stays within the parity tolerance of the projected oracle Q.  Then
batches, direction shards, the bilinear form, the standalone entry point, determinism, graph replay, a long relaxation and
the C++ driver."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bilinear_ref as BR
import conserve_ref as CR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-12
TOL32 = 5e-6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (the HIP path has no fallback)")
    return torch


def _op(bfsm, shape, n_gl, n_sph, prec=64, conserve=True, small=True, exact=False, hermitian=False, shard=None, max_batch=0,
        sph=None):
    c = bfsm.reference_constants()
    op = bfsm.HIPBoltzmannOperator(bfsm.GaussLegendreQuadrature(n_gl, 0.0, c["R"]), sph or bfsm.SphericalDesign(n_sph),
                                   *shape, c["gamma"], c["b_gamma"], c["L"])
    op.setPrecision(prec)
    op.setSmallPath(small)
    op.setExactReductions(exact, hermitian)
    op.setConservation(conserve)
    if shard:
        op.setDirectionShard(*shard)
    if max_batch:
        op.setMaxBatch(max_batch)
    op.initialize()
    return op


def _input(bfsm, shape, seed=0):
    if shape[0] == shape[1] == shape[2]:
        return bfsm.perturbed_input(bfsm.bkw_solution(shape[0])[0], seed=0x5EED + seed)
    return np.random.default_rng(1 + seed).random(shape) + 0.1


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eval(torch, op, f_h):
    f = _dev(torch, f_h)
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.computeCollision(Q, f)
    return Q.cpu().numpy()


def _L():
    import bfsm
    return bfsm.reference_constants()["L"]


def _assert_conserved(P, scale_from, what=""):
    m = np.abs(CR.moments(P, _L()))
    s = CR.moment_scale(scale_from, _L())
    assert np.all(m <= 1e-12 * s), (what, m / s)


ROUTES = [
    ((16, 16, 16), 64, {}, 8, 32),
    ((16, 16, 16), 64, {"small": False}, 8, 32),
    ((32, 32, 32), 64, {}, 4, 12),
    ((64, 64, 64), 64, {}, 2, 6),
    ((64, 64, 64), 64, {"exact": True}, 2, 6),
    ((64, 64, 64), 64, {"exact": True, "hermitian": True}, 2, 6),
    ((128, 128, 128), 32, {}, 3, 6),          # three radial nodes: one would cancel its gain against the loss in fp32
    ((12, 8, 20), 64, {}, 2, 6),
    ((160, 4, 6), 64, {}, 2, 6),
    ((160, 4, 6), 32, {}, 2, 6),
]


@pytest.mark.parametrize("shape,prec,kw,n_gl,n_sph", ROUTES)
def test_routes_conserve_and_match_the_projected_oracle(torch_cuda, oracle, shape, prec, kw, n_gl, n_sph):
    import bfsm
    f_h = _input(bfsm, shape)
    op0 = _op(bfsm, shape, n_gl, n_sph, prec, conserve=False, **kw)
    opc = _op(bfsm, shape, n_gl, n_sph, prec, conserve=True, **kw)
    Q0 = _eval(torch_cuda, op0, f_h)
    Qc = _eval(torch_cuda, opc, f_h)
    op0.destroy()
    opc.destroy()
    _assert_conserved(Qc, Q0, shape)
    d0 = np.abs(CR.moments(Q0, _L())) / CR.moment_scale(Q0, _L())
    assert d0[[0, 4]].max() > 1e-10, d0                  # the unflagged defect is at truncation level, far above rounding
    scale = np.abs(Q0).max()
    assert np.abs(Qc - CR.project(Q0, _L())).max() <= 1e-13 * scale
    c = bfsm.reference_constants()
    ref = oracle.collide(f_h, oracle.gauss_legendre(n_gl, 0.0, c["R"]), oracle.spherical_design(n_sph), c["gamma"],
                         c["b_gamma"], c["L"])
    want = CR.project(ref, _L())
    assert np.abs(Qc - want).max() <= (10 * TOL64 if prec == 64 else TOL32) * np.abs(ref).max()


def test_batch_members_are_the_single_evaluations(torch_cuda):
    import bfsm
    torch = torch_cuda
    nv, nb = 32, 3
    f0 = bfsm.bkw_solution(nv)[0]
    fs_h = np.stack([bfsm.perturbed_input(f0, seed=100 + i, amp=0.05 * (i + 1)) for i in range(nb)])
    op = _op(bfsm, (nv,) * 3, 4, 12, max_batch=nb)
    fs = _dev(torch, fs_h)
    Qb = torch.empty_like(fs)
    op.computeCollisionBatch(Qb, fs, nb)
    Qb_h = Qb.cpu().numpy()
    single = torch.empty(nv ** 3, dtype=torch.float64, device="cuda")
    for i in range(nb):
        op(single, fs[i].reshape(-1).contiguous())
        assert np.array_equal(single.cpu().numpy().reshape(nv, nv, nv), Qb_h[i])
        _assert_conserved(Qb_h[i], Qb_h[i], i)
    op.destroy()


@pytest.mark.parametrize("P", [2, 3])
def test_direction_shards_sum_to_the_flagged_full_handle(torch_cuda, P):
    import bfsm
    torch = torch_cuda
    nv, n_gl, n_sph = 32, 4, 12
    f_h = _input(bfsm, (nv,) * 3)
    full = _op(bfsm, (nv,) * 3, n_gl, n_sph)
    want = _eval(torch, full, f_h)
    full.destroy()
    f = _dev(torch, f_h)
    fs = torch.stack([f, f * 1.1]).contiguous()
    fb = torch.empty_like(fs)
    ranks = [_op(bfsm, (nv,) * 3, n_gl, n_sph, shard=bfsm.shard_range(n_gl * n_sph, r, P), max_batch=2) for r in range(P)]
    sums = {k: torch.zeros_like(f) for k in ("collide", "gain_finish")}
    sum_b = torch.zeros_like(fs)
    Q = torch.empty_like(f)
    for r, op in enumerate(ranks):
        op.collidePartial(Q, f, r == 0)
        sums["collide"] += Q
        op.gainPartial(f)
        op.finishPartial(Q, f, r == 0)
        sums["gain_finish"] += Q
        op.collideBatchPartial(fb, fs, 2, r == 0)
        sum_b += fb
    torch.cuda.synchronize()
    for op in ranks:
        op.destroy()
    for k, s in sums.items():
        assert np.abs(s.cpu().numpy() - want).max() <= 1e-13 * np.abs(want).max(), k
    assert np.abs(sum_b[0].cpu().numpy() - want).max() <= 1e-13 * np.abs(want).max()
    _assert_conserved(sum_b[1].cpu().numpy(), sum_b[1].cpu().numpy())


class _Rule:
    def __init__(self, x, y, z, w):
        self.x, self.y, self.z, self.w = x, y, z, w

    def getx(self):
        return self.x

    def gety(self):
        return self.y

    def getz(self):
        return self.z

    def getWeights(self):
        return self.w

    def getNumberOfPoints(self):
        return len(self.w)


def test_bilinear_and_linearized_forms(torch_cuda):
    import bfsm
    torch = torch_cuda
    shape = (32, 32, 32)
    c = bfsm.reference_constants()
    rng = np.random.default_rng(4)
    g_h, f_h = rng.random(shape) + 0.1, rng.random(shape) + 0.1
    sph = _Rule(*BR.random_rule(7, seed=5))
    op = _op(bfsm, shape, 2, 7, sph=sph)
    g, f = _dev(torch, g_h), _dev(torch, f_h)
    Q = torch.empty_like(f)
    op.computeBilinearCollision(Q, g, f)
    got = Q.cpu().numpy()
    gl = bfsm.GaussLegendreQuadrature(2, 0.0, c["R"])
    ref = BR.collide_bilinear(g_h, f_h, (gl.getNodes(), gl.getWeights()), (sph.x, sph.y, sph.z, sph.w), c["gamma"],
                              c["b_gamma"], c["L"])
    assert np.abs(got - CR.project(ref, c["L"])).max() <= 10 * TOL64 * np.abs(ref).max()
    _assert_conserved(got, ref)
    Lh = torch.empty_like(f)
    op.linearizedCollision(Lh, f, g)
    op.destroy()
    _assert_conserved(Lh.cpu().numpy(), Lh.cpu().numpy())


def test_standalone_entry_point(torch_cuda):
    import bfsm
    torch = torch_cuda
    shape = (32, 32, 32)
    f_h = _input(bfsm, shape)
    op0 = _op(bfsm, shape, 4, 12, conserve=False)
    opc = _op(bfsm, shape, 4, 12, conserve=True)
    f = _dev(torch, f_h)
    Q0, Qc = torch.empty_like(f), torch.empty_like(f)
    op0.computeCollision(Q0, f)
    opc.computeCollision(Qc, f)
    op0.conserve(Q0)
    torch.cuda.synchronize()
    assert torch.equal(Q0, Qc)
    Q2 = Q0.clone()
    op0.conserve(Q2)
    torch.cuda.synchronize()
    assert (Q2 - Q0).abs().max().item() <= 1e-15 * Q0.abs().max().item()
    L = op0._lib
    assert L.bfsm_conserve_async(op0._h, None, 1, None) == 1
    for nb in (0, 2, -1):
        assert L.bfsm_conserve_async(op0._h, ctypes.c_void_p(Q0.data_ptr()), nb, None) == 1
        assert b"n_batch" in L.bfsm_last_error(op0._h)
    op0.destroy()
    opc.destroy()


def test_flagged_evaluation_is_deterministic(torch_cuda):
    import bfsm
    torch = torch_cuda
    op = _op(bfsm, (64, 64, 64), 2, 6)
    f = _dev(torch, _input(bfsm, (64, 64, 64)))
    Q = torch.empty_like(f)
    op.computeCollision(Q, f)
    first = Q.clone()
    for _ in range(20):
        op.computeCollision(Q, f)
        assert torch.equal(Q, first)
    op.destroy()


def test_flagged_evaluation_replays_in_a_graph(torch_cuda):
    import bfsm
    torch = torch_cuda
    shape = (32, 32, 32)
    f0 = _input(bfsm, shape)
    op = _op(bfsm, shape, 4, 12)
    f = _dev(torch, f0)
    Q, Qg = torch.empty_like(f), torch.empty_like(f)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op.computeCollisionAsync(Qg, f, side.cuda_stream)          # first call outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        op.computeCollisionAsync(Qg, f, torch.cuda.current_stream().cuda_stream)
    for scale in (1.0, 0.5):
        f.copy_(torch.from_numpy(f0 * scale))
        Qg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        op.computeCollision(Q, f)
        assert torch.equal(Q, Qg)
    op.destroy()


def _maxwellian(v, rho, u, T):
    vx, vy, vz = np.meshgrid(v, v, v, indexing="ij")
    d2 = (vx - u[0]) ** 2 + (vy - u[1]) ** 2 + (vz - u[2]) ** 2
    return rho / (2 * np.pi * T) ** 1.5 * np.exp(-d2 / (2 * T))


def _relax(torch, bfsm, conserve, f0_h, steps, dt):
    op = _op(bfsm, f0_h.shape, 16, 32, conserve=conserve)
    f = _dev(torch, f0_h.reshape(-1))
    work = tuple(torch.empty_like(f) for _ in range(3))
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(steps):
        bfsm.ssp_rk3_step(op, f, dt, work, stream)
    torch.cuda.synchronize()
    op.destroy()
    return f.cpu().numpy().reshape(f0_h.shape)


def test_long_relaxation_conserves_and_reaches_the_right_maxwellian(torch_cuda):
    """SSP-RK3 at N = 32 from a two-Maxwellian with bulk velocity to t = 30.  With the flag, mass, momentum and energy stay
    put to rounding, so the Maxwellian the run relaxes to is the one of the initial moments; without it, that Maxwellian
    drifts.  The flagged f is within 1e-3 (relative L2) of it: the unweighted projection adds sum_k lambda_k psi_k, which
    is largest at the corners of the box, so the discrete equilibrium of PQ carries a small polynomial tail (INTEGRATION.md
    section 6); the unflagged run ends closer in L2 at t = 30 (its moment drift is still ~1e-4)."""
    import bfsm
    nv, L = 32, _L()
    dv = 2 * L / nv
    v = -L + dv / 2 + np.arange(nv) * dv
    f0 = 0.5 * _maxwellian(v, 1.0, (1.0, 0.5, 0.0), 1.0) + 0.5 * _maxwellian(v, 1.0, (-1.0, 0.0, 0.5), 0.8)
    vx, vy, vz = np.meshgrid(v, v, v, indexing="ij")
    v2 = vx * vx + vy * vy + vz * vz

    def mom(f):
        return f.sum(), np.array([(f * vx).sum(), (f * vy).sum(), (f * vz).sum()]), (f * v2).sum()

    m0, p0, e0 = mom(f0)
    u = p0 / m0
    T = (e0 / m0 - u @ u) / 3
    M = _maxwellian(v, 1.0, u, T)
    M *= m0 / M.sum()                            # the Maxwellian of the initial moments, with the datum's discrete mass

    def dist(a, b):
        return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))

    def own_maxwellian(f):          # the Maxwellian of f's own discrete moments
        m, p, e = mom(f)
        uf = p / m
        Mf = _maxwellian(v, 1.0, uf, (e / m - uf @ uf) / 3)
        return Mf * (m / Mf.sum())

    def drifts(f):
        m, p, e = mom(f)
        return abs(m - m0) / m0, float(np.abs(p - p0).max() / m0), abs(e - e0) / e0, dist(f, M), dist(own_maxwellian(f), M)

    fc = _relax(torch_cuda, bfsm, True, f0, 300, 0.1)
    fu = _relax(torch_cuda, bfsm, False, f0, 300, 0.1)
    c, u_ = drifts(fc), drifts(fu)
    msg = f"(mass, momentum, energy drift, |f - M|, |M(f) - M|): flagged {c}; unflagged {u_}"
    assert c[0] <= 1e-12 and c[2] <= 1e-12 and c[1] <= 1e-12, msg
    assert c[4] < u_[4] and c[4] <= 1e-12, msg       # the equilibrium the flagged run heads for is the right one
    assert c[3] <= 1e-3, msg


def test_cpp_relaxation_driver_conserves(torch_cuda):
    pkg = os.path.join(os.path.dirname(HERE), "boltzmann-fourier-spectral-method_amd")
    exe = os.path.join(pkg, "bkw_relax_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", pkg, "-s", "bkw_relax_hip"])
    out = subprocess.run([exe, "--Nv", "32", "--Ngl", "16", "--Ns", "32", "--steps", "10", "--exact-reductions", "--conserve",
                          "--design-dir", os.path.join(pkg, "data", "sph_design")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    l2 = float(re.search(r"L2 error vs exact BKW: (\S+)", out.stdout).group(1))
    mass = float(re.search(r"relative mass drift: (\S+)", out.stdout).group(1))
    energy = float(re.search(r"relative energy drift: (\S+)", out.stdout).group(1))
    mom = float(re.search(r"momentum drift \|p1 - p0\| / m0: (\S+)", out.stdout).group(1))
    assert l2 < 2e-4 and mass <= 1e-12 and energy <= 1e-12 and mom <= 1e-12, out.stdout
