"""-m gpu: the symmetric form Qs(g,f) = Q(g,f) + Q(f,g) (include/bfsm.h, bfsm_collide_symmetric*) on the MI355X.

Every entry of tests/symmetric_cases.py against tests/symmetric_ref.py (two reference evaluations on the full rule), after the
case has shown on the reference alone that it tells the operator from a single merged pass; a rule without antipodal symmetry
on Hermitian handles; the launch-sequence variants (profiled launches show the reduce route); shards, BFSM_FLAG_CONSERVE,
determinism, independence of the handle's call history, graph replay, argument errors and the C++ mirror.  Bounds as in
tests/test_gpu_bilinear.py: fp64 1e-12, fp32 5e-6, relative to max|reference|.  Every case prints its measured error."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bilinear_cases as BC
import bilinear_ref as BR
import conserve_ref as CR
import symmetric_cases as SC
import symmetric_ref as SR
from test_emu_symmetric import B_GAMMA, GAMMA, L_BOX, TEETH, TOL32, TOL64, _rel, _tol, fields, gauss_legendre, gpu_inputs
from test_gpu_bilinear import _Rule, _dev, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


class _GL:
    """Radial quadrature object (the interface HIPBoltzmannOperator reads) over given nodes and weights."""
    def __init__(self, nodes, weights):
        self.nodes, self.weights = nodes, weights

    def getNodes(self):
        return self.nodes

    def getWeights(self):
        return self.weights

    def getNumberOfPoints(self):
        return len(self.nodes)


def _make(shape, prec, mode, gl, sph, shard=None, max_chunk=0, max_batch=0, profile=False, conserve=False):
    import bfsm
    shape = (shape,) * 3 if isinstance(shape, int) else shape
    op = bfsm.HIPBoltzmannOperator(_GL(*gl), _Rule(*sph), *shape, GAMMA, B_GAMMA, L_BOX)
    op.setPrecision(prec)
    if shard:
        op.setDirectionShard(*shard)
    op.setMaxChunk(max_chunk)
    op.setMaxBatch(max_batch)
    op.setProfiling(profile)
    op.setExactReductions(mode != "faithful", hermitian=(mode == "hermitian"))
    op.setConservation(conserve)
    op.initialize()
    return op


def _symmetric(torch, op, g_h, f_h):
    g, f = _dev(torch, g_h), _dev(torch, f_h)
    Q = torch.full_like(f, float("nan"))
    torch.cuda.synchronize()
    op.computeSymmetricCollision(Q, g, f)
    return Q.cpu().numpy()


@pytest.mark.parametrize("c", SC.CASES, ids=SC.cid)
def test_case_matches_reference(torch_cuda, c):
    inp = gpu_inputs(c)
    tol = _tol(c.prec)
    print(f"{SC.cid(c)} [{c.ka}]: a single merged pass lies at {inp['away']:.2e} from the reference")
    assert inp["away"] >= TEETH * tol, "this case could not see a missing exchanged product"
    op = _make(c.shape, c.prec, c.mode, inp["gl"], inp["sph"])
    cnt = op.counters()
    got = _symmetric(torch_cuda, op, inp["g"], inp["f"])
    op.destroy()
    if isinstance(c.shape, int):
        assert cnt.antipodal_merged == (0 if c.mode == "faithful" else 1) and cnt.n_dirs == c.n_gl * c.sph_eff
    err = _rel(got, inp["ref"])
    print(f"{SC.cid(c)}: Qs(g,f) max rel err {err:.2e} (bound {tol:.0e})")
    assert err <= tol


@pytest.mark.parametrize("n,prec", SC.VARIANT_SIZES)
def test_rule_without_antipodal_symmetry_on_a_hermitian_handle(torch_cuda, n, prec):
    """Nothing is merged: every direction of the odd rule in both operand orders, on the stored half of the planes."""
    g, f = fields((n, n, n), seed=n + 1)
    gl, sph = gauss_legendre(2), BR.random_rule(5, seed=n)
    op = _make(n, prec, "hermitian", gl, sph)
    assert op.counters().antipodal_merged == 0
    got = _symmetric(torch_cuda, op, g, f)
    op.destroy()
    err = _rel(got, SR.collide_symmetric(g, f, gl, sph, GAMMA, B_GAMMA, L_BOX))
    print(f"N={n} fp{prec} hermitian, odd rule: max rel err {err:.2e}")
    assert err <= _tol(prec)


@pytest.mark.parametrize("v", SC.VARIANTS, ids=lambda v: f"N{v.n}-fp{v.prec}-{v.kind}")
def test_launch_sequence_variants(torch_cuda, v):
    from bfsm import capi
    torch = torch_cuda
    c = SC.case(v.n, v.prec, "hermitian")
    inp = gpu_inputs(c)
    op = _make(v.n, v.prec, "hermitian", inp["gl"], inp["sph"], shard=v.shard, max_chunk=v.max_chunk, max_batch=v.max_batch,
               profile=True)
    g, f = _dev(torch, inp["g"]), _dev(torch, inp["f"])
    Q = torch.full_like(f, float("nan"))
    torch.cuda.synchronize()
    op.collideSymmetricPartial(Q, g, f, True)
    op.synchronize()
    cnt = op.counters()
    launches = tuple(cnt.kernel_launches)
    op.destroy()
    if v.shard is None:
        ref = inp["ref"]
    else:
        # a shard of a merged plan is a range of EFFECTIVE directions (make_plan: b * sph_eff / n_sph), each an antipodal pair:
        # the reference on the half rule with doubled weights over that range (Qs of a pair = 2 w_s [P_s(g,f) + P_s(f,g)])
        e0, e1 = (b * c.sph_eff // c.n_sph for b in v.shard)
        ref = SR.collide_symmetric(inp["g"], inp["f"], inp["gl"], SR.half_rule_doubled(inp["sph"]), GAMMA, B_GAMMA, L_BOX,
                                   dir_range=(e0, e1))
    err = _rel(Q.cpu().numpy(), ref)
    print(f"N={v.n} fp{v.prec} {v.kind}: {cnt.n_chunks} chunks, launches {launches}, max rel err {err:.2e}")
    assert cnt.n_chunks == v.chunks
    assert launches[capi.KERNEL_NAMES.index("reduce")] == v.reduce
    kn_own = v.n != 64                       # KN's own launch is booked under gain_inv
    assert launches[capi.KERNEL_NAMES.index("gain_inv")] == 2 * cnt.n_chunks * (2 if kn_own else 1)
    assert launches[capi.KERNEL_NAMES.index("gain_fwd")] == 1 and launches[capi.KERNEL_NAMES.index("tail")] == 2
    assert err <= _tol(v.prec)


@pytest.mark.parametrize("n,prec", SC.VARIANT_SIZES)
def test_three_uneven_shards_sum_to_the_reference(torch_cuda, n, prec):
    torch = torch_cuda
    c = SC.case(n, prec, "hermitian")
    inp = gpu_inputs(c)
    g, f = _dev(torch, inp["g"]), _dev(torch, inp["f"])
    total = np.zeros_like(inp["f"])
    for rank, rng in enumerate(BC.shards(c.n_gl * c.n_sph)):
        op = _make(n, prec, "hermitian", inp["gl"], inp["sph"], shard=rng)
        Q = torch.empty_like(f)
        torch.cuda.synchronize()
        op.collideSymmetricPartial(Q, g, f, with_loss=(rank == 1))
        op.synchronize()
        total += Q.cpu().numpy()
        op.destroy()
    err = _rel(total, inp["ref"])
    print(f"N={n} fp{prec}: shards {BC.shards(c.n_gl * c.n_sph)} summed, max rel err {err:.2e}")
    assert err <= _tol(prec)


@pytest.mark.parametrize("shape,prec,mode", [(24, 64, "hermitian"), (24, 32, "hermitian"), ((12, 8, 20), 64, "faithful")])
def test_conserve_projects_the_symmetric_form_once(torch_cuda, shape, prec, mode):
    """Q = P Qs: the five discrete invariants vanish to 1e-12 of their scale (tests/test_gpu_conserve.py), and Q is
    conserve_ref.project of the reference."""
    c = SC.case(shape, prec, mode)
    inp = gpu_inputs(c)
    op = _make(shape, prec, mode, inp["gl"], inp["sph"], conserve=True)
    got = _symmetric(torch_cuda, op, inp["g"], inp["f"])
    op.destroy()
    m, s = np.abs(CR.moments(got, L_BOX)), CR.moment_scale(got, L_BOX)
    print(f"{SC.cid(c)} conserve: moments / scale {m / s}")
    assert np.all(m <= 1e-12 * s), m / s
    assert _rel(got, CR.project(np.asarray(inp["ref"]), L_BOX)) <= _tol(prec)


def test_history_does_not_change_a_bit(torch_cuda):
    """Repeated calls are bitwise equal; on a faithful handle computeCollision and computeBilinearCollision in between do not
    change the symmetric result; on an exact + Hermitian handle Q(f,f) is bitwise the same before and after a symmetric call
    (the doubled segment sums and slabs are shared safely)."""
    torch = torch_cuda
    c = SC.case(24, 64, "hermitian")
    inp = gpu_inputs(c)
    g, f = _dev(torch, inp["g"]), _dev(torch, inp["f"])
    for mode in ("faithful", "hermitian"):
        op = _make(24, 64, mode, inp["gl"], inp["sph"])
        first, Q, tmp = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
        op.computeSymmetricCollision(first, g, f)
        for _ in range(3):
            op.computeSymmetricCollision(Q, g, f)
            assert torch.equal(Q, first)
        q0, q1 = torch.empty_like(f), torch.empty_like(f)
        op.computeCollision(q0, f)
        if mode == "faithful":
            op.computeBilinearCollision(tmp, g, f)
        else:
            assert op._lib.bfsm_collide_bilinear(op._h, ctypes.c_void_p(tmp.data_ptr()), ctypes.c_void_p(g.data_ptr()),
                                                 ctypes.c_void_p(f.data_ptr())) == 2          # still BFSM_ERR_UNSUPPORTED
        op.computeSymmetricCollision(Q, g, f)
        assert torch.equal(Q, first), mode
        op.computeCollision(q1, f)
        assert torch.equal(q0, q1), mode
        op.destroy()


def test_capture_and_replay_on_one_stream(torch_cuda):
    torch = torch_cuda
    c = SC.case(24, 64, "hermitian")
    inp = gpu_inputs(c)
    op = _make(24, 64, "hermitian", inp["gl"], inp["sph"])
    g, f = _dev(torch, inp["g"]), _dev(torch, inp["f"])
    Q, Qg = torch.empty_like(f), torch.empty_like(f)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op.computeSymmetricCollisionAsync(Qg, g, f, side.cuda_stream)         # first call outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        op.computeSymmetricCollisionAsync(Qg, g, f, torch.cuda.current_stream().cuda_stream)
    for scale in (1.0, -0.5):
        g.copy_(torch.from_numpy(np.asarray(inp["g"]) * scale))
        Qg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        op.computeSymmetricCollision(Q, g, f)
        assert torch.equal(Q, Qg)
        assert _rel(Qg.cpu().numpy(), scale * np.asarray(inp["ref"])) <= TOL64
    op.destroy()


def test_argument_errors(torch_cuda):
    torch = torch_cuda
    c = SC.case(24, 64, "hermitian")
    inp = gpu_inputs(c)
    G = 24 ** 3
    op = _make(24, 64, "hermitian", inp["gl"], inp["sph"])
    part = _make(24, 64, "hermitian", inp["gl"], inp["sph"], shard=(0, 8))
    lib = op._lib
    buf = torch.zeros(3 * G, dtype=torch.float64, device="cuda")
    p = lambda off: ctypes.c_void_p(buf.data_ptr() + 8 * off)
    for args, needle in [((None, p(G), p(2 * G)), b"null"), ((p(0), None, p(2 * G)), b"null"), ((p(0), p(G), None), b"null"),
                         ((p(G - 1), p(G), p(2 * G)), b"overlap"), ((p(2 * G - 1), p(0), p(G)), b"overlap"),
                         ((p(0), p(0), p(2 * G)), b"overlap")]:
        assert lib.bfsm_collide_symmetric_partial_async(op._h, *args, 1, None) == 1, args
        assert needle in lib.bfsm_last_error(op._h), lib.bfsm_last_error(op._h)
    assert lib.bfsm_collide_symmetric_async(part._h, p(0), p(G), p(2 * G), None) == 1
    assert b"owns all directions" in lib.bfsm_last_error(part._h)
    assert lib.bfsm_collide_symmetric(part._h, p(0), p(G), p(2 * G)) == 1
    torch.cuda.synchronize()
    assert not buf.any()
    got = _symmetric(torch, op, inp["g"], inp["f"])                          # the handle still works
    assert _rel(got, inp["ref"]) <= TOL64
    op.destroy()
    part.destroy()


def test_cpp_mirror(torch_cuda, tmp_path):
    """tests/host/test_symmetric_mirror.cpp: computeSymmetricCollision of BoltzmannOperator<HIP_Backend> on an exact + Hermitian
    handle against its own computeCollision (Qs(f,f) = 2 Q(f,f)) and against the polarization identity."""
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "boltzmann-fourier-spectral-method_amd")
    exe = str(tmp_path / "test_symmetric_mirror")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I", os.path.join(pkg, "host"), "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "test_symmetric_mirror.cpp"),
                           os.path.join(pkg, "host", "HIPBoltzmannOperator.cpp"), os.path.join(pkg, "host", "Quadratures", "SphericalDesign.cpp"),
                           "-L" + pkg, "-lbfsm_hip", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.run([exe, os.path.join(pkg, "data", "sph_design")], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "symmetric mirror checks passed" in out.stdout
