"""-m gpu: every route of the size-generic path (csrc/bfsm_generic.hpp) on the MI355X, case by case from
tests/generic_cases.py, whose coverage of the selection code tests/test_generic_routes.py checks on the CPU.

  * Q(f,f) of every case against the oracle (symmetry-free input, gamma = 0.5, b_gamma = 0.3), with profiling on: the
    kernel_launches of bfsm_get_counters must equal the case's -- the proof that the GPU took the route the case claims;
  * Q(g,f) of the cases that run the bilinear producers, against tests/bilinear_ref.py with a rule without antipodal
    symmetry;
  * two direction shards (the loss term on rank 0) summed against the oracle, and a batch of two members against the
    single evaluations;
  * bfsm_fft3d forward and backward against numpy.fft for every supported length (72 even lengths 4..256 with factors
    <= 13) on the x pass, in the plane (y and z) and on the per-axis y / z passes, batch of 2, both precisions.
    Worst error over the sweep relative to max|ref|, measured on the MI355X: fp64 forward 5.35e-16 at (4, 14, 234),
    backward 6.52e-16 at (4, 14, 210); fp32 forward 1.87e-7 at (4, 88, 4), backward 2.05e-7 at (4, 14, 126).  FFT_TOL
    is 3x those (the one generic box the suite transformed before had a forward bound of 4e-15 in fp64).

Tolerances of the operator as in test_gpu_parity.py: fp64 1e-12 max|Q_ref|, fp32 5e-6."""
import numpy as np
import pytest

import bilinear_ref as BR
import generic_cases as GC

pytestmark = pytest.mark.gpu

TOL64 = 1e-12
TOL32 = 5e-6
TOL = {64: TOL64, 32: TOL32}
FFT_TOL = {(64, -1): 1.6e-15, (64, +1): 1.95e-15, (32, -1): 5.6e-7, (32, +1): 6.1e-7}     # (precision, sign)
GAMMA, B_GAMMA, L_BOX = 0.5, 0.3, 11.0

CASE_PRECS = [pytest.param(c, p, id=f"{c.name}-fp{p}") for c in GC.CASES for p in c.precs]


def _with(op_name):
    return [pytest.param(c, p, id=f"{c.name}-fp{p}") for c in GC.CASES if op_name in c.ops for p in c.precs]


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


def _op(bfsm, case, prec, shard=None, max_batch=0, profile=False, sph=None):
    c = bfsm.reference_constants()
    op = bfsm.HIPBoltzmannOperator(bfsm.GaussLegendreQuadrature(case.n_gl, 0.0, c["R"]),
                                   sph if sph is not None else bfsm.SphericalDesign(case.n_sph), *case.shape, GAMMA, B_GAMMA, L_BOX)
    op.setPrecision(prec)
    if shard:
        op.setDirectionShard(*shard)
    if case.max_chunk:
        op.setMaxChunk(case.max_chunk)
    op.setMaxBatch(max_batch)
    op.setProfiling(profile)
    op.initialize()
    return op


def _oracle(oracle, case, f_h, dir_range=None):
    import bfsm
    c = bfsm.reference_constants()
    return oracle.collide(f_h, oracle.gauss_legendre(case.n_gl, 0.0, c["R"]), oracle.spherical_design(case.n_sph), GAMMA,
                          B_GAMMA, L_BOX, dir_range=dir_range)


def _field(case, seed=0):
    return np.random.default_rng(sum(case.shape) + seed).random(case.shape) + 0.1      # no symmetry at all


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("case,prec", CASE_PRECS)
def test_whole_operator_takes_the_declared_route(torch_cuda, oracle, case, prec):
    import bfsm
    torch = torch_cuda
    f_h = _field(case)
    op = _op(bfsm, case, prec, profile=True)
    f = torch.from_numpy(f_h).cuda()
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op(Q, f)
    launches = tuple(op.counters().kernel_launches)
    op.destroy()
    assert launches == tuple(case.launches[prec]), (case.name, prec, launches)
    err = _rel(Q.cpu().numpy(), _oracle(oracle, case, f_h))
    print(f"{case.name} fp{prec}: launches {launches}, Q(f,f) rel err {err:.2e}")
    assert err <= TOL[prec]


@pytest.mark.parametrize("case,prec", _with("bilinear"))
def test_bilinear_producers(torch_cuda, case, prec):
    import bfsm
    torch = torch_cuda
    rng = np.random.default_rng(sum(case.shape) + 7)
    g_h, f_h = rng.random(case.shape) + 0.1, rng.random(case.shape) + 0.1
    sph = _Rule(*BR.random_rule(case.n_sph, seed=sum(case.shape)))
    op = _op(bfsm, case, prec, sph=sph)
    g, f = torch.from_numpy(g_h).cuda(), torch.from_numpy(f_h).cuda()
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.computeBilinearCollision(Q, g, f)
    op.destroy()
    c = bfsm.reference_constants()
    gl = bfsm.GaussLegendreQuadrature(case.n_gl, 0.0, c["R"])
    ref = BR.collide_bilinear(g_h, f_h, (gl.getNodes(), gl.getWeights()), (sph.x, sph.y, sph.z, sph.w), GAMMA, B_GAMMA, L_BOX)
    err = _rel(Q.cpu().numpy(), ref)
    print(f"{case.name} fp{prec}: Q(g,f) rel err {err:.2e}")
    assert err <= TOL[prec]


@pytest.mark.parametrize("case,prec", _with("shards"))
def test_direction_shards_sum_to_the_oracle(torch_cuda, oracle, case, prec):
    import bfsm
    torch = torch_cuda
    f_h = _field(case, 1)
    f = torch.from_numpy(f_h).cuda()
    tot = torch.zeros_like(f)
    for r, rng_ in enumerate(GC.shard_ranges(case)):
        op = _op(bfsm, case, prec, shard=rng_)
        Q = torch.empty_like(f)
        torch.cuda.synchronize()
        op.collidePartial(Q, f, r == 0)
        op.synchronize()
        tot += Q
        op.destroy()
    assert _rel(tot.cpu().numpy(), _oracle(oracle, case, f_h)) <= TOL[prec]


@pytest.mark.parametrize("case,prec", _with("batch"))
def test_batch_of_two_is_the_single_evaluations(torch_cuda, oracle, case, prec):
    """Members with different values through one bfsm_collide_batch: on the fused sequence all members go through every
    launch together, elsewhere one after the other -- bitwise the single evaluations either way."""
    import bfsm
    torch = torch_cuda
    fs = np.stack([_field(case, 2), 0.3 + _field(case, 3) ** 2])
    single = _op(bfsm, case, prec)
    ones = []
    for i in range(2):
        f = torch.from_numpy(fs[i]).cuda()
        Q = torch.empty_like(f)
        torch.cuda.synchronize()
        single(Q, f)
        ones.append(Q)
    single.destroy()
    op = _op(bfsm, case, prec, max_batch=2)
    fb = torch.from_numpy(fs).cuda()
    Qb = torch.empty_like(fb)
    op.computeCollisionBatch(Qb, fb, 2)
    op.destroy()
    for i in range(2):
        assert torch.equal(Qb[i], ones[i]), (case.name, prec, i)
        assert _rel(Qb[i].cpu().numpy(), _oracle(oracle, case, fs[i])) <= TOL[prec]


@pytest.mark.parametrize("prec", [64, 32])
def test_fft3d_every_length_and_placement(torch_cuda, prec):
    import bfsm
    torch = torch_cuda
    cdtype = torch.complex128 if prec == 64 else torch.complex64
    rng = np.random.default_rng(prec)
    worst = {-1: (0.0, None), +1: (0.0, None)}
    lengths = GC.fft_lengths()
    assert len(lengths) == 72
    case = GC.Case("fft", None, 1, 6, 0, (prec,), (), (), {})
    for n in lengths:
        for box in GC.fft_boxes(n):
            op = _op(bfsm, case._replace(shape=box), prec)
            a = rng.standard_normal((2,) + box) + 1j * rng.standard_normal((2,) + box)
            if prec == 32:
                a = a.astype(np.complex64).astype(np.complex128)       # the transform's own error, not the input's rounding
            for sign, ref in ((-1, np.fft.fftn(a, axes=(1, 2, 3))), (+1, np.fft.ifftn(a, axes=(1, 2, 3)) * a[0].size)):
                d = torch.from_numpy(a).to(cdtype).cuda()
                op.fft3d(d, 2, sign)
                err = _rel(d.cpu().numpy().astype(np.complex128), ref)
                if err > worst[sign][0]:
                    worst[sign] = (err, box)
                assert err <= FFT_TOL[(prec, sign)], (box, prec, sign, err)
            op.destroy()
    print(f"fp{prec} fft3d worst rel err: forward {worst[-1][0]:.2e} at {worst[-1][1]}, backward {worst[1][0]:.2e} at {worst[1][1]}")
