"""-m gpu: the bilinear collision operator Q(g,f) on every fused cube and precision (tests/bilinear_cases.py) on the MI355X.

Each case of the table against the numpy restatement tests/bilinear_ref.py, with a rule without antipodal symmetry, g != f
and gamma != 0; before the GPU runs, the case shows on the CPU that it can see g and f exchanged in the gain.  g == f as one
pointer against the oracle's Q(f,f).  At the cfg3 and cfg5 geometries and N = 80 in single precision, the launch-sequence
variants: several chunks, the separate and the fused slab reduce (profiled launches), direction shards and a handle created
for batches.  The linearized operator against the reference.  Bounds as in tests/test_gpu_bilinear.py: fp64 1e-12, fp32
5e-6, relative to max|Q_ref|.  Every case prints its measured error."""
import numpy as np
import pytest

import bilinear_cases as BC
import bilinear_ref as BR
from test_gpu_bilinear import L_BOX, TOL32, TOL64, _Rule, _bilinear, _dev, _fields, _rel, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

GAMMA, B_GAMMA = 0.5, 0.3
R_MAX = 10.0
# 1000 x the bound: how far the reference with the gain's arguments exchanged must lie from the reference
DISCRIMINATION = 1000.0

_INPUTS = {}


def _tol(prec):
    return TOL64 if prec == 64 else TOL32


def _inputs(n, n_gl, n_sph, refs=True):
    """g, f and the quadratures of a cube case; refs: with the references Q(g,f) and Q(f,g) and the distance of the swapped
    gain.  Computed once for both precisions and every test of the size."""
    key = (n, n_gl, n_sph)
    if key not in _INPUTS:
        import bfsm
        g, f = _fields((n, n, n), seed=n)
        gl = bfsm.GaussLegendreQuadrature(n_gl, 0.0, R_MAX)
        _INPUTS[key] = dict(g=g, f=f, gl=gl, glq=(gl.getNodes(), gl.getWeights()), sph=BR.random_rule(n_sph, seed=n))
    inp = _INPUTS[key]
    if refs and "gf" not in inp:
        g, f, glq, sph = inp["g"], inp["f"], inp["glq"], inp["sph"]
        inp["gf"] = BR.collide_bilinear(g, f, glq, sph, GAMMA, B_GAMMA, L_BOX)
        inp["fg"] = BR.collide_bilinear(f, g, glq, sph, GAMMA, B_GAMMA, L_BOX)
        # the gain with its arguments exchanged, the loss term g Lambda[f] kept: Q(f,g) + f Lambda[g] - g Lambda[f]
        lam_f, lam_g = (BR.loss_rate(h, glq, GAMMA, B_GAMMA, L_BOX) for h in (f, g))
        inp["swap"] = _rel(inp["fg"] + f * lam_g - g * lam_f, inp["gf"])
    return inp


def _case_inputs(n, prec):
    c = BC.cube(n, prec)
    return _inputs(c.n, c.n_gl, c.n_sph)


def _make(bfsm, n, prec, inp, shard=None, max_chunk=0, max_batch=0, profile=False):
    op = bfsm.HIPBoltzmannOperator(inp["gl"], _Rule(*inp["sph"]), n, n, n, GAMMA, B_GAMMA, L_BOX)
    op.setPrecision(prec)
    if shard:
        op.setDirectionShard(*shard)
    op.setMaxChunk(max_chunk)
    op.setMaxBatch(max_batch)
    op.setProfiling(profile)
    op.initialize()
    return op


def _cid(c):
    return f"N{c.n}-fp{c.prec}"


@pytest.mark.parametrize("case", BC.CUBES, ids=_cid)
def test_cube_matches_reference(torch_cuda, case):
    import bfsm
    inp = _inputs(case.n, case.n_gl, case.n_sph)
    tol = _tol(case.prec)
    print(f"N={case.n} fp{case.prec} [{case.geometry}]: reference with the gain's arguments exchanged at {inp['swap']:.2e}")
    assert inp["swap"] >= DISCRIMINATION * tol, "this case could not see g and f exchanged in the gain"
    op = _make(bfsm, case.n, case.prec, inp)
    got = _bilinear(torch_cuda, op, inp["g"], inp["f"])
    op.destroy()
    err = _rel(got, inp["gf"])
    print(f"N={case.n} fp{case.prec}: Q(g,f) max rel err {err:.2e} (bound {tol:.0e})")
    assert err <= tol


@pytest.mark.parametrize("case", BC.CUBES, ids=_cid)
def test_same_pointer_is_the_oracle_operator(torch_cuda, oracle, case):
    """g == f as one pointer: the one-transform branch of Pipeline::collide_bilinear."""
    import bfsm
    torch = torch_cuda
    inp = _inputs(case.n, case.n_gl, case.n_sph, refs=False)
    op = _make(bfsm, case.n, case.prec, inp)
    f = _dev(torch, inp["f"])
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.computeBilinearCollision(Q, f, f)
    got = Q.cpu().numpy()
    op.destroy()
    ref = oracle.collide(inp["f"], inp["glq"], inp["sph"], GAMMA, B_GAMMA, L_BOX)
    err = _rel(got, ref)
    print(f"N={case.n} fp{case.prec}: Q(f,f) through one pointer, max rel err {err:.2e} against the oracle")
    assert err <= _tol(case.prec)


@pytest.mark.parametrize("v", BC.VARIANTS, ids=lambda v: f"N{v.n}-fp{v.prec}-chunk{v.max_chunk}")
def test_chunks_and_reduce_route(torch_cuda, v):
    """Several chunks across radial-node boundaries with the separate Reduce launch (more than 8 slabs), and one chunk
    with the reduce fused into the tail; the profiled launches show which route the call took."""
    import bfsm
    from bfsm import capi
    inp = _case_inputs(v.n, v.prec)
    op = _make(bfsm, v.n, v.prec, inp, max_chunk=v.max_chunk, profile=True)
    got = _bilinear(torch_cuda, op, inp["g"], inp["f"])
    cnt = op.counters()
    launches = tuple(cnt.kernel_launches)
    op.destroy()
    err = _rel(got, inp["gf"])
    print(f"N={v.n} fp{v.prec} max_chunk={v.max_chunk}: {cnt.n_chunks} chunks, launches {launches}, max rel err {err:.2e}")
    assert cnt.n_chunks == v.chunks
    assert launches[capi.KERNEL_NAMES.index("reduce")] == v.reduce
    assert launches[capi.KERNEL_NAMES.index("gain_inv")] == cnt.n_chunks
    assert err <= _tol(v.prec)


@pytest.mark.parametrize("n,prec", BC.VARIANT_SIZES)
def test_three_uneven_shards_sum_to_the_reference(torch_cuda, n, prec):
    import bfsm
    torch = torch_cuda
    inp = _case_inputs(n, prec)
    c = BC.cube(n, prec)
    g, f = _dev(torch, inp["g"]), _dev(torch, inp["f"])
    total = np.zeros_like(inp["f"])
    for rank, rng in enumerate(BC.shards(c.n_gl * c.n_sph)):
        op = _make(bfsm, n, prec, inp, shard=rng)
        Q = torch.empty_like(f)
        torch.cuda.synchronize()
        op.collideBilinearPartial(Q, g, f, with_loss=(rank == 0))
        op.synchronize()
        total += Q.cpu().numpy()
        op.destroy()
    err = _rel(total, inp["gf"])
    print(f"N={n} fp{prec}: shards {BC.shards(c.n_gl * c.n_sph)} summed, max rel err {err:.2e}")
    assert err <= _tol(prec)


@pytest.mark.parametrize("n,prec", BC.BATCH_SIZES)
def test_single_call_on_a_batch_handle(torch_cuda, n, prec):
    import bfsm
    inp = _case_inputs(n, prec)
    op = _make(bfsm, n, prec, inp, max_batch=BC.MAX_BATCH)
    got = _bilinear(torch_cuda, op, inp["g"], inp["f"])
    op.destroy()
    err = _rel(got, inp["gf"])
    print(f"N={n} fp{prec} max_batch={BC.MAX_BATCH}: max rel err {err:.2e}")
    assert err <= _tol(prec)


@pytest.mark.parametrize("n,prec", [(64, 64), (128, 32)])
def test_linearized_collision_matches_reference(torch_cuda, n, prec):
    """L_f[h] = Q(f,h) + Q(h,f) with h = the case's g, against the two reference terms; the bound is relative to the
    larger of them."""
    import bfsm
    torch = torch_cuda
    inp = _case_inputs(n, prec)
    op = _make(bfsm, n, prec, inp)
    f, h = _dev(torch, inp["f"]), _dev(torch, inp["g"])
    Lh = torch.empty_like(f)
    torch.cuda.synchronize()
    op.linearizedCollision(Lh, f, h)
    got = Lh.cpu().numpy()
    op.destroy()
    ref = inp["fg"] + inp["gf"]          # Q(f,h) + Q(h,f)
    scale = max(np.abs(inp["fg"]).max(), np.abs(inp["gf"]).max())
    err = float(np.abs(got - ref).max() / scale)
    print(f"N={n} fp{prec}: linearized operator max rel err {err:.2e}")
    assert err <= _tol(prec)
