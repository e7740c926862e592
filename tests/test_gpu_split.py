"""-m gpu: the gain / loss split (include/bfsm.h, bfsm_collide_split*, bfsm_loss_rate_async) on the MI355X.

Qgain and nu against the numpy restatement tests/split_ref.py on every fused cube in both precisions (the (N, precision) pairs
of tests/bilinear_cases.py) and on the routes of the size-generic path; the assembled Qgain - f nu against bfsm_collide on the
same handle; the exact / Hermitian gain modes; direction shards with nu = NULL; batches; the bilinear form; the loss-only
call; a BFSM_FLAG_CONSERVE handle; argument checks; graph capture.  Every case: 2 radial nodes x a 3-point rule without
antipodal symmetry (6 directions), gamma = 0.5, b_gamma = 0.3, L = 11, random fields.  Bounds as in tests/test_gpu_bilinear.py:
fp64 1e-12, fp32 5e-6, each relative to max|ref| of the array compared.  Every case prints its measured errors."""
import numpy as np
import pytest

import bilinear_cases as BC
import bilinear_ref as BR
import split_ref as SR
from test_gpu_bilinear import L_BOX, TOL32, TOL64, _Rule, _dev, _fields, _rel, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

GAMMA, B_GAMMA = 0.5, 0.3
R_MAX = 10.0
N_GL, N_SPH = 2, 3
N_DIRS = N_GL * N_SPH
DISCRIMINATION = 1000.0
EPS = float(np.finfo(np.float64).eps)
FLAG_EXACT, FLAG_HERMITIAN = 2, 4

_INPUTS = {}


def _tol(prec):
    return TOL64 if prec == 64 else TOL32


def _shape(n):
    return (n, n, n) if np.isscalar(n) else tuple(n)


def _inputs(n, design=None):
    """g, f, the quadratures and the references (Qgain, nu) of Q(f,f) for a grid, computed once per grid and rule.
    design: points of a shipped (antipodal) spherical design instead of the random rule."""
    import bfsm
    shape = _shape(n)
    key = (shape, design)
    if key not in _INPUTS:
        g, f = _fields(shape, seed=sum(shape))
        gl = bfsm.GaussLegendreQuadrature(N_GL, 0.0, R_MAX)
        if design:
            sd = bfsm.SphericalDesign(design)
            sph = (sd.getx(), sd.gety(), sd.getz(), sd.getWeights())
        else:
            sph = BR.random_rule(N_SPH, seed=sum(shape))
        inp = dict(g=g, f=f, gl=gl, glq=(gl.getNodes(), gl.getWeights()), sph=sph)
        inp["Qgain"], inp["nu"] = SR.split(f, f, inp["glq"], sph, GAMMA, B_GAMMA, L_BOX)
        _INPUTS[key] = inp
    return _INPUTS[key]


def _make(n, prec, inp, shard=None, max_batch=0, exact=False, hermitian=False, conserve=False):
    import bfsm
    op = bfsm.HIPBoltzmannOperator(inp["gl"], _Rule(*inp["sph"]), *_shape(n), GAMMA, B_GAMMA, L_BOX)
    op.setPrecision(prec)
    if shard:
        op.setDirectionShard(*shard)
    op.setMaxBatch(max_batch)
    op.setExactReductions(exact, hermitian)
    op.setConservation(conserve)
    op.initialize()
    return op


def _split(torch, op, f_h):
    f = _dev(torch, f_h)
    Qg, nu = torch.empty_like(f), torch.empty_like(f)
    torch.cuda.synchronize()
    op.computeCollisionSplit(Qg, nu, f)
    return Qg.cpu().numpy(), nu.cpu().numpy()


def _check(label, Qg, nu, Qg_ref, nu_ref, tol):
    eg, en = _rel(Qg, Qg_ref), _rel(nu, nu_ref)
    print(f"{label}: Qgain max rel err {eg:.2e}, nu max rel err {en:.2e} (bound {tol:.0e})")
    assert eg <= tol and en <= tol


def _cid(c):
    return f"N{c.n}-fp{c.prec}"


@pytest.mark.parametrize("case", BC.CUBES, ids=_cid)
def test_cube_split_matches_reference(torch_cuda, case):
    inp = _inputs(case.n)
    tol = _tol(case.prec)
    f, Qg_ref, nu_ref = inp["f"], inp["Qgain"], inp["nu"]
    d_nu, d_q = _rel(f * nu_ref, nu_ref), _rel(Qg_ref - f * nu_ref, Qg_ref)
    print(f"N={case.n} fp{case.prec}: f nu lies {d_nu:.2e} from nu, Qgain - f nu lies {d_q:.2e} from Qgain")
    assert d_nu >= DISCRIMINATION * tol and d_q >= DISCRIMINATION * tol, "this case could not see a product with f or a subtraction"
    op = _make(case.n, case.prec, inp)
    Qg, nu = _split(torch_cuda, op, f)
    op.destroy()
    _check(f"N={case.n} fp{case.prec}", Qg, nu, Qg_ref, nu_ref, tol)


@pytest.mark.parametrize("shape,prec", [
    ((12, 8, 20), 64), ((12, 8, 20), 32),     # fused sequence of the size-generic path
    ((160, 4, 6), 64),                        # the 8-line kernels
    ((20, 20, 20), 64),                       # plane kernel route
])
def test_generic_path_split_matches_reference(torch_cuda, shape, prec):
    inp = _inputs(shape)
    op = _make(shape, prec, inp)
    Qg, nu = _split(torch_cuda, op, inp["f"])
    op.destroy()
    _check(f"{shape} fp{prec}", Qg, nu, inp["Qgain"], inp["nu"], _tol(prec))


@pytest.mark.parametrize("n", [32, (12, 8, 20)])
def test_assembled_split_is_bfsm_collide_on_the_same_handle(torch_cuda, n):
    """Qgain - f nu against Q of bfsm_collide: the same transforms, so the only difference is one fused or unfused
    multiply-add per point."""
    torch = torch_cuda
    inp = _inputs(n)
    op = _make(n, 64, inp)
    f = _dev(torch, inp["f"])
    Q = torch.empty_like(f)
    op.computeCollision(Q, f)
    Qg, nu = _split(torch, op, inp["f"])
    op.destroy()
    diff = np.abs(Qg - inp["f"] * nu - Q.cpu().numpy())
    bound = 4 * EPS * (np.abs(Qg) + np.abs(inp["f"] * nu))
    print(f"{_shape(n)}: max |Qgain - f nu - Q| / bound = {float((diff / bound).max()):.3f}")
    assert bool((diff <= bound).all())


@pytest.mark.parametrize("hermitian", [False, True], ids=["exact", "exact-hermitian"])
@pytest.mark.parametrize("n", [16, 32, 64])
def test_gain_modes(torch_cuda, n, hermitian):
    inp = _inputs(n, design=12)
    op = _make(n, 64, inp, exact=True, hermitian=hermitian)
    cnt = op.counters()
    assert cnt.exact_reductions == 1 and cnt.antipodal_merged == 1
    Qg, nu = _split(torch_cuda, op, inp["f"])
    op.destroy()
    _check(f"N={n} exact{'|hermitian' if hermitian else ''}", Qg, nu, inp["Qgain"], inp["nu"], TOL64)


@pytest.mark.parametrize("n,prec", [(64, 64), (128, 32)])
def test_three_uneven_shards(torch_cuda, n, prec):
    torch = torch_cuda
    inp = _inputs(n)
    f = _dev(torch, inp["f"])
    total = np.zeros_like(inp["f"])
    nu0 = None
    for rank, rng in enumerate(BC.shards(N_DIRS)):
        op = _make(n, prec, inp, shard=rng)
        Qg = torch.empty_like(f)
        torch.cuda.synchronize()
        if rank == 0:
            nu = torch.empty_like(f)
            op.collideSplitBatchPartial(Qg, nu, f, 1, True)
            op.synchronize()
            nu0 = nu.cpu().numpy()
        else:
            op.collideSplitBatchPartial(Qg, None, f, 1, False)           # nu = NULL
            op.synchronize()
            again, sentinel = torch.empty_like(f), torch.full_like(f, -7.25)
            op.collideSplitBatchPartial(again, sentinel, f, 1, False)    # a nu buffer is not touched without the loss term
            op.synchronize()
            assert bool((sentinel == -7.25).all()) and torch.equal(again, Qg)
        total += Qg.cpu().numpy()
        op.destroy()
    _check(f"N={n} fp{prec} shards {BC.shards(N_DIRS)}", total, nu0, inp["Qgain"], inp["nu"], _tol(prec))


@pytest.mark.parametrize("n", [16, (12, 8, 20)])
def test_batch_members_are_the_single_calls(torch_cuda, n):
    torch = torch_cuda
    inp = _inputs(n)
    members = [inp["f"], inp["g"], 0.5 * (inp["f"] + inp["g"]) ** 2]
    op = _make(n, 64, inp, max_batch=3)
    fs = _dev(torch, np.stack(members))
    Qg, nu = torch.empty_like(fs), torch.empty_like(fs)
    torch.cuda.synchronize()
    op.collideSplitBatchPartial(Qg, nu, fs, 3, True)
    op.synchronize()
    for i, m in enumerate(members):
        Qi, nui = _split(torch, op, m)                                   # the same handle
        assert np.array_equal(Qg[i].cpu().numpy(), Qi) and np.array_equal(nu[i].cpu().numpy(), nui), i
        Qg_ref, nu_ref = (inp["Qgain"], inp["nu"]) if i == 0 else SR.split(m, m, inp["glq"], inp["sph"], GAMMA, B_GAMMA, L_BOX)
        _check(f"{_shape(n)} member {i}", Qi, nui, Qg_ref, nu_ref, TOL64)
    op.destroy()


@pytest.mark.parametrize("n,prec", [(32, 64), (80, 32), ((12, 8, 20), 64)])
def test_bilinear_split(torch_cuda, n, prec):
    torch = torch_cuda
    inp = _inputs(n)
    Qg_ref, nu_ref = SR.split(inp["g"], inp["f"], inp["glq"], inp["sph"], GAMMA, B_GAMMA, L_BOX)
    op = _make(n, prec, inp)
    g, f = _dev(torch, inp["g"]), _dev(torch, inp["f"])
    Qg, nu = torch.empty_like(f), torch.empty_like(f)
    torch.cuda.synchronize()
    op.computeBilinearSplit(Qg, nu, g, f)
    op.destroy()
    _check(f"{_shape(n)} fp{prec} Q(g,f)", Qg.cpu().numpy(), nu.cpu().numpy(), Qg_ref, nu_ref, _tol(prec))


def test_bilinear_split_on_an_exact_handle_is_unsupported(torch_cuda):
    import bfsm
    torch = torch_cuda
    inp = _inputs(32, design=12)
    op = _make(32, 64, inp, exact=True)
    g, f = _dev(torch, inp["g"]), _dev(torch, inp["f"])
    Qg, nu = torch.full_like(f, 7.0), torch.full_like(f, -3.0)
    with pytest.raises(bfsm.BfsmError) as e:
        op.collideBilinearSplitPartial(Qg, nu, g, f, True)
    assert e.value.code == 2 and "EXACT_REDUCTIONS" in str(e.value)
    torch.cuda.synchronize()
    assert bool((Qg == 7.0).all()) and bool((nu == -3.0).all())
    op.destroy()


@pytest.mark.parametrize("n,prec", [(16, 64), (64, 64), (128, 32), ((12, 8, 20), 64)])
def test_loss_rate_alone(torch_cuda, n, prec):
    torch = torch_cuda
    inp = _inputs(n)
    tol = _tol(prec)
    g_ref = BR.loss_rate(inp["g"], inp["glq"], GAMMA, B_GAMMA, L_BOX)
    op = _make(n, prec, inp, max_batch=2)
    fs = _dev(torch, np.stack([inp["f"], inp["g"]]))
    nu = torch.empty_like(fs)
    torch.cuda.synchronize()
    op.lossRate(nu, fs, 2)
    op.synchronize()
    got = nu.cpu().numpy()
    op.destroy()
    shard = _make(n, prec, inp, shard=(1, 3))                            # the loss does not depend on the shard
    f = _dev(torch, inp["f"])
    nu1 = torch.empty_like(f)
    torch.cuda.synchronize()
    shard.lossRate(nu1, f)
    shard.synchronize()
    shard.destroy()
    errs = (_rel(got[0], inp["nu"]), _rel(got[1], g_ref), _rel(nu1.cpu().numpy(), inp["nu"]))
    print(f"{_shape(n)} fp{prec}: nu max rel err, batch of 2: {errs[0]:.2e} {errs[1]:.2e}; shard handle: {errs[2]:.2e} (bound {tol:.0e})")
    assert max(errs) <= tol


def test_conserve_flag_does_not_touch_the_split(torch_cuda):
    torch = torch_cuda
    inp = _inputs(32)
    plain, cons = _make(32, 64, inp), _make(32, 64, inp, conserve=True)
    Qg, nu = _split(torch, plain, inp["f"])
    Qg_c, nu_c = _split(torch, cons, inp["f"])
    assert np.array_equal(Qg, Qg_c) and np.array_equal(nu, nu_c)
    f = _dev(torch, inp["f"])
    PQ = torch.empty_like(f)
    cons.computeCollision(PQ, f)                                         # the flag handle's combined call: P Q
    Q = _dev(torch, Qg - inp["f"] * nu)                                  # assembled by the caller, then projected
    torch.cuda.synchronize()
    plain.conserve(Q)
    plain.synchronize()
    plain.destroy()
    cons.destroy()
    # the assembled Q differs from the combined one by at most 4 eps (|Qgain| + |f nu|) per point; P is an orthogonal
    # projection (norm 1 in l2), so the difference stays far inside the project's fp64 bound relative to max|Q|
    err = float((Q - PQ).abs().max() / PQ.abs().max())
    print(f"N=32: P(Qgain - f nu) against the flag handle's bfsm_collide: max rel diff {err:.2e}")
    assert err <= TOL64


def test_argument_checks(torch_cuda):
    import bfsm
    torch = torch_cuda
    inp = _inputs(16)
    f = _dev(torch, inp["f"])
    a, b = torch.empty_like(f), torch.empty_like(f)
    op = _make(16, 64, inp)
    for args in ((a, a, f), (f, b, f), (a, f, f)):                       # Qgain / nu, Qgain / f, nu / f overlap
        with pytest.raises(bfsm.BfsmError) as e:
            op.computeCollisionSplit(*args)
        assert e.value.code == 1
    fs = torch.empty(2 * f.numel(), dtype=f.dtype, device=f.device)
    with pytest.raises(bfsm.BfsmError) as e:                             # n_batch > max_batch
        op.collideSplitBatchPartial(torch.empty_like(fs), torch.empty_like(fs), fs, 2, True)
    assert e.value.code == 1
    with pytest.raises(bfsm.BfsmError) as e:
        op.lossRate(torch.empty_like(fs), fs, 2)
    assert e.value.code == 1
    op.destroy()
    shard = _make(16, 64, inp, shard=(0, 3))
    with pytest.raises(bfsm.BfsmError) as e:                             # a shard through the non-partial entry
        shard.computeCollisionSplit(a, b, f)
    assert e.value.code == 1
    with pytest.raises(bfsm.BfsmError) as e:
        shard.computeCollisionSplitAsync(a, b, f)
    assert e.value.code == 1
    shard.destroy()


def test_async_form_replays_in_a_graph(torch_cuda):
    torch = torch_cuda
    inp = _inputs(32)
    op = _make(32, 64, inp)
    f = _dev(torch, inp["f"])
    Qg, nu, Qg_c, nu_c = (torch.empty_like(f) for _ in range(4))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op.computeCollisionSplitAsync(Qg_c, nu_c, f, side.cuda_stream)   # first call outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        op.computeCollisionSplitAsync(Qg_c, nu_c, f, torch.cuda.current_stream().cuda_stream)
    for scale in (1.0, 0.5):
        f.copy_(torch.from_numpy(inp["f"] * scale))
        Qg_c.zero_()
        nu_c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        op.computeCollisionSplit(Qg, nu, f)
        assert torch.equal(Qg, Qg_c) and torch.equal(nu, nu_c)
    op.destroy()
