"""-m gpu: the bilinear collision operator Q(g,f) (include/bfsm.h, bfsm_collide_bilinear*) on the MI355X.

Against the numpy restatement tests/bilinear_ref.py with a spherical rule WITHOUT antipodal symmetry (so the convention
A1 <- g, A2 <- f is what is checked), on every kernel route; identities at full size; shards, errors, graph capture and
the linearized operator.  Tolerances as in test_gpu_parity.py: fp64 1e-12 max|Q_ref|, fp32 5e-6."""
import numpy as np
import pytest

import bilinear_ref as BR

pytestmark = pytest.mark.gpu

TOL64 = 1e-12
TOL32 = 5e-6
L_BOX = 11.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (the HIP path has no fallback)")
    return torch


class _Rule:
    """Spherical quadrature object (the interface HIPBoltzmannOperator reads) over given points and weights."""
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


def _op(bfsm, shape, gl, sph, precision=64, gamma=0.5, b_gamma=0.3, shard=None, small_path=True, exact=False):
    op = bfsm.HIPBoltzmannOperator(gl, sph, *shape, gamma, b_gamma, L_BOX)
    op.setPrecision(precision)
    if shard:
        op.setDirectionShard(*shard)
    op.setSmallPath(small_path)
    op.setExactReductions(exact)
    op.initialize()
    return op


def _fields(shape, seed=3):
    rng = np.random.default_rng(seed)
    return rng.random(shape) + 0.1, rng.random(shape) + 0.1      # g, f: no symmetry at all


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bilinear(torch, op, g_h, f_h):
    g, f = _dev(torch, g_h), _dev(torch, f_h)
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.computeBilinearCollision(Q, g, f)
    return Q.cpu().numpy()


def _collide(torch, op, f_h):
    f = _dev(torch, f_h)
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.computeCollision(Q, f)
    return Q.cpu().numpy()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("shape,prec,small", [
    ((16, 16, 16), 64, True), ((16, 16, 16), 64, False), ((16, 16, 16), 32, True),
    ((24, 24, 24), 64, True), ((32, 32, 32), 64, True), ((48, 48, 48), 64, True),
    ((24, 24, 24), 32, True), ((32, 32, 32), 32, True), ((48, 48, 48), 32, True),
    ((12, 8, 20), 64, True), ((12, 8, 20), 32, True),
    ((160, 4, 6), 64, True),                 # long x lines: the 8-lines-per-workgroup x-line kernel
    ((4, 14, 160), 64, True),                # ... and the 8-line z pass that forms the phase
])
def test_matches_reference_non_antipodal_rule(torch_cuda, shape, prec, small):
    import bfsm
    g, f = _fields(shape, seed=sum(shape))
    gl = bfsm.GaussLegendreQuadrature(2, 0.0, 10.0)
    sph = _Rule(*BR.random_rule(7, seed=sum(shape)))
    op = _op(bfsm, shape, gl, sph, prec, small_path=small)
    got = _bilinear(torch_cuda, op, g, f)
    op.destroy()
    ref = BR.collide_bilinear(g, f, (gl.getNodes(), gl.getWeights()), (sph.x, sph.y, sph.z, sph.w), 0.5, 0.3, L_BOX)
    assert _rel(got, ref) <= (TOL64 if prec == 64 else TOL32)


@pytest.mark.parametrize("nv", [32, 64])
def test_g_equal_f_is_bfsm_collide(torch_cuda, nv):
    import bfsm
    f_h = bfsm.perturbed_input(bfsm.bkw_solution(nv)[0])
    op = _op(bfsm, (nv, nv, nv), bfsm.GaussLegendreQuadrature(4, 0.0, 10.0), bfsm.SphericalDesign(12), gamma=0.0,
             b_gamma=1 / (4 * np.pi))
    torch = torch_cuda
    f = _dev(torch, f_h)
    Q, Qb, Qs = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    op.computeCollision(Q, f)
    op.computeBilinearCollision(Qb, f.clone(), f)       # two spectra of equal values
    op.computeBilinearCollision(Qs, f, f)               # the same pointer
    op.destroy()
    for got in (Qb, Qs):
        rel = float((got - Q).abs().max() / Q.abs().max())
        print(f"N={nv}: Q(f,f) bilinear vs bfsm_collide: max rel diff {rel:.2e}, bitwise {bool(torch.equal(got, Q))}")
        # bitwise at N = 32; at N = 64 the bilinear KA (conj(alpha) plane re-read instead of held) rounds differently in
        # the last place: 1.06e-15 measured, so a 2e-15 bound
        assert rel <= 2e-15


def _full_size_identities(torch, bfsm, nv, n_gl, n_sph, prec, tol):
    f0 = bfsm.bkw_solution(nv)[0]
    f_h = bfsm.perturbed_input(f0)
    g_h = bfsm.perturbed_input(f0, seed=0xB11) * (1.0 + 0.3 * np.linspace(-1.0, 1.0, nv))[None, :, None]
    c = bfsm.reference_constants()
    gl = bfsm.GaussLegendreQuadrature(n_gl, 0.0, c["R"])
    op = bfsm.HIPBoltzmannOperator(gl, bfsm.SphericalDesign(n_sph), nv, nv, nv, c["gamma"], c["b_gamma"], c["L"])
    op.setPrecision(prec)
    op.initialize()
    gf = _bilinear(torch, op, g_h, f_h)
    fg = _bilinear(torch, op, f_h, g_h)
    qs = _collide(torch, op, f_h + g_h)
    qf = _collide(torch, op, f_h)
    qg = _collide(torch, op, g_h)
    op.destroy()
    lam_f = BR.loss_rate(f_h, (gl.getNodes(), gl.getWeights()), c["gamma"], c["b_gamma"], c["L"])
    lam_g = BR.loss_rate(g_h, (gl.getNodes(), gl.getWeights()), c["gamma"], c["b_gamma"], c["L"])
    scale = np.abs(gf + g_h * lam_f).max() + np.abs(g_h * lam_f).max()   # gain and loss magnitudes
    # antipodal design: the gain is symmetric, so Q(g,f) - Q(f,g) = f Lambda[g] - g Lambda[f]
    anti = np.abs((gf - fg) - (f_h * lam_g - g_h * lam_f)).max() / scale
    # polarization against the library's own Q(f,f)
    pol = np.abs((gf + fg) - (qs - qf - qg)).max() / scale
    print(f"N={nv} fp{prec} {n_gl}x{n_sph}: antisymmetry {anti:.2e}, polarization {pol:.2e} (relative to gain + loss)")
    assert anti <= tol and pol <= tol


def test_full_size_cfg3_identities(torch_cuda):
    import bfsm
    _full_size_identities(torch_cuda, bfsm, 64, 16, 48, 64, TOL64)


def test_full_size_n128_fp32_identities(torch_cuda):
    import bfsm
    _full_size_identities(torch_cuda, bfsm, 128, 2, 48, 32, TOL32)


@pytest.mark.parametrize("shape", [(32, 32, 32), (12, 8, 20)])
def test_direction_shards_sum_to_the_full_handle(torch_cuda, shape):
    import bfsm
    torch = torch_cuda
    g_h, f_h = _fields(shape, seed=5)
    gl = bfsm.GaussLegendreQuadrature(2, 0.0, 10.0)
    sph = _Rule(*BR.random_rule(7, seed=2))
    B = 14
    full = _op(bfsm, shape, gl, sph)
    ref = _bilinear(torch, full, g_h, f_h)
    full.destroy()
    g, f = _dev(torch, g_h), _dev(torch, f_h)
    parts = []
    for rank, rng in enumerate(((0, 6), (6, B))):
        op = _op(bfsm, shape, gl, sph, shard=rng)
        Q = torch.empty_like(f)
        op.collideBilinearPartial(Q, g, f, with_loss=(rank == 0))
        op.synchronize()
        parts.append(Q.cpu().numpy())
        op.destroy()
    assert _rel(parts[0] + parts[1], ref) <= TOL64


def test_exact_reduction_handle_is_unsupported_and_leaves_Q(torch_cuda):
    import bfsm
    torch = torch_cuda
    op = _op(bfsm, (32, 32, 32), bfsm.GaussLegendreQuadrature(2, 0.0, 10.0), bfsm.SphericalDesign(6), exact=True)
    g_h, f_h = _fields((32, 32, 32))
    g, f = _dev(torch, g_h), _dev(torch, f_h)
    Q = torch.full_like(f, 7.0)
    with pytest.raises(bfsm.BfsmError) as e:
        op.computeBilinearCollision(Q, g, f)
    assert e.value.code == 2 and "EXACT_REDUCTIONS" in str(e.value)
    torch.cuda.synchronize()
    assert bool((Q == 7.0).all())
    with pytest.raises(bfsm.BfsmError) as e:
        op.collideBilinearPartial(Q, g, f, True)
    assert e.value.code == 2
    op.destroy()


def test_Q_aliasing_an_input_is_invalid(torch_cuda):
    import bfsm
    torch = torch_cuda
    op = _op(bfsm, (16, 16, 16), bfsm.GaussLegendreQuadrature(2, 0.0, 10.0), bfsm.SphericalDesign(6))
    g_h, f_h = _fields((16, 16, 16))
    g, f = _dev(torch, g_h), _dev(torch, f_h)
    for args in ((g, g, f), (f, g, f)):
        with pytest.raises(bfsm.BfsmError) as e:
            op.computeBilinearCollision(*args)
        assert e.value.code == 1
    op.destroy()


def test_async_form_replays_in_a_graph(torch_cuda):
    import bfsm
    torch = torch_cuda
    shape = (32, 32, 32)
    g0, f0 = _fields(shape, seed=8)
    op = _op(bfsm, shape, bfsm.GaussLegendreQuadrature(2, 0.0, 10.0), _Rule(*BR.random_rule(7)))
    g, f = _dev(torch, g0), _dev(torch, f0)
    Q, Qg = torch.empty_like(f), torch.empty_like(f)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op.computeBilinearCollisionAsync(Qg, g, f, side.cuda_stream)      # first call outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        op.computeBilinearCollisionAsync(Qg, g, f, torch.cuda.current_stream().cuda_stream)
    for scale in (1.0, 0.5):
        g.copy_(torch.from_numpy(g0 * scale))
        Qg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        op.computeBilinearCollision(Q, g, f)
        assert torch.equal(Q, Qg)
    op.destroy()


def test_linearized_collision_is_the_central_difference(torch_cuda):
    """Q is quadratic, so (Q(f + eps h) - Q(f - eps h)) / (2 eps) = Q(f,h) + Q(h,f) = L_f[h] up to rounding."""
    import bfsm
    torch = torch_cuda
    nv = 32
    f_h = bfsm.perturbed_input(bfsm.bkw_solution(nv)[0])
    h_h = bfsm.perturbed_input(bfsm.bkw_solution(nv)[0], seed=0xABC) - f_h * 0.95
    op = _op(bfsm, (nv, nv, nv), bfsm.GaussLegendreQuadrature(4, 0.0, 10.0), _Rule(*BR.random_rule(9)), gamma=0.0,
             b_gamma=1 / (4 * np.pi))
    eps = 1e-3
    f, h = _dev(torch, f_h), _dev(torch, h_h)
    Lh = torch.empty_like(f)
    op.linearizedCollision(Lh, f, h)
    fd = (_collide(torch, op, f_h + eps * h_h) - _collide(torch, op, f_h - eps * h_h)) / (2 * eps)
    got = Lh.cpu().numpy()
    tmp = torch.empty_like(f)
    Lh2 = torch.empty_like(f)
    op.linearizedCollision(Lh2, f, h, tmp=tmp)                       # caller-owned temporary
    op.destroy()
    assert _rel(got, fd) <= 1e-10
    assert np.array_equal(Lh2.cpu().numpy(), got)
