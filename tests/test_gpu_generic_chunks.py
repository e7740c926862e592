"""-m gpu: chunkings of the size-generic path's fused sequence on the MI355X, entry by entry from
tests/generic_chunk_cases.py, whose declared groups and properties tests/test_generic_chunks.py proves on the CPU from the
launch recorder: later chunks that launch more plane-accumulate groups than the first (the slab buffer must hold them),
fewer, max_chunk = 1, a last chunk of one direction, and the default as the baseline.

  * Q(f,f) of every entry against the oracle for the entry's directions (symmetry-free input, gamma = 0.5, b_gamma = 0.3,
    L = 11), with profiling on: n_chunks and the gain_fwd launch count of bfsm_get_counters must equal the entry's -- the
    proof that the GPU ran the plan the entry claims.  Chunkings differ from one another in the order of the sums, so each is
    compared with the oracle, not with another chunking;
  * on the entries with a later chunk of more groups: the shard plus its complement, summed; a batch of two on a
    max_batch = 2 handle, each member bitwise the single call on the same handle; Q(g,f) against tests/bilinear_ref.py and
    the gain / loss split against tests/split_ref.py with a rule without antipodal symmetry.

Tolerances as in test_gpu_parity.py: fp64 1e-12 max|ref|, fp32 5e-6."""
import numpy as np
import pytest

import bilinear_ref as BR
import generic_chunk_cases as CC
import split_ref as SR
from test_gpu_generic_routes import B_GAMMA, GAMMA, L_BOX, TOL, _Rule, _rel, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

GAIN_FWD = 3          # BFSM_K_GAIN_FWD
CASE_PRECS = [pytest.param(c, p, id=f"{c.name}-fp{p}") for c in CC.CASES for p in c.precs]
MORE_PRECS = [pytest.param(c, p, id=f"{c.name}-fp{p}") for c in CC.CASES if CC.MORE in c.props for p in c.precs]

_REFS = {}


def _gl(bfsm, case):
    return bfsm.GaussLegendreQuadrature(case.n_gl, 0.0, bfsm.reference_constants()["R"])


def _op(bfsm, case, prec, shard=None, max_batch=0, profile=False, sph=None):
    op = bfsm.HIPBoltzmannOperator(_gl(bfsm, case), sph if sph is not None else bfsm.SphericalDesign(case.n_sph), *case.shape,
                                   GAMMA, B_GAMMA, L_BOX)
    op.setPrecision(prec)
    shard = shard or (case.dir_range if case.dir_range != CC.ALL else None)
    if shard:
        op.setDirectionShard(*shard)
    if case.max_chunk:
        op.setMaxChunk(case.max_chunk)
    op.setMaxBatch(max_batch)
    op.setProfiling(profile)
    op.initialize()
    return op


def _field(case, seed=0):
    return np.random.default_rng(sum(case.shape) + seed).random(case.shape) + 0.1      # no symmetry at all


def _oracle(oracle, case, f_h, dir_range="case"):
    """The oracle's Q (gain of dir_range, full loss), once per (box, rule, directions, field)."""
    import bfsm
    if dir_range == "case":
        dir_range = case.dir_range if case.dir_range != CC.ALL else None
    key = (case.shape, case.n_gl, case.n_sph, dir_range, f_h.tobytes())
    if key not in _REFS:
        c = bfsm.reference_constants()
        _REFS[key] = oracle.collide(f_h, oracle.gauss_legendre(case.n_gl, 0.0, c["R"]), oracle.spherical_design(case.n_sph), GAMMA,
                                    B_GAMMA, L_BOX, dir_range=dir_range)
    return _REFS[key]


def _partial(torch, op, f, with_loss=True):
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.collidePartial(Q, f, with_loss)
    op.synchronize()
    return Q


@pytest.mark.parametrize("case,prec", CASE_PRECS)
def test_chunking_runs_its_plan_and_matches_the_oracle(torch_cuda, oracle, case, prec):
    import bfsm
    torch = torch_cuda
    f_h = _field(case)
    op = _op(bfsm, case, prec, profile=True)
    Q = _partial(torch, op, torch.from_numpy(f_h).cuda())
    cnt = op.counters()
    n_chunks, gain_fwd = cnt.n_chunks, cnt.kernel_launches[GAIN_FWD]
    op.destroy()
    err = _rel(Q.cpu().numpy(), _oracle(oracle, case, f_h))
    print(f"{case.name} fp{prec}: {n_chunks} chunks, {gain_fwd} gain_fwd launches, Q(f,f) rel err {err:.2e}")
    assert n_chunks == len(case.groups) and gain_fwd == len(case.groups)
    assert err <= TOL[prec]


@pytest.mark.parametrize("case,prec", MORE_PRECS)
def test_shard_and_complement_sum_to_the_oracle(torch_cuda, oracle, case, prec):
    """The chunked shard with the loss term plus the directions it leaves out (none for an entry that owns all)."""
    import bfsm
    torch = torch_cuda
    f_h = _field(case, 1)
    f = torch.from_numpy(f_h).cuda()
    op = _op(bfsm, case, prec)
    tot = _partial(torch, op, f)
    op.destroy()
    rest = CC.complement(case)
    if rest:
        op = _op(bfsm, case, prec, shard=rest)
        tot += _partial(torch, op, f, with_loss=False)
        op.destroy()
        ref = _oracle(oracle, case, f_h, dir_range=None)
    else:
        ref = _oracle(oracle, case, f_h)
    err = _rel(tot.cpu().numpy(), ref)
    print(f"{case.name} fp{prec}: shard + complement rel err {err:.2e}")
    assert err <= TOL[prec]


@pytest.mark.parametrize("case,prec", MORE_PRECS)
def test_batch_of_two_is_the_single_call_on_the_same_handle(torch_cuda, oracle, case, prec):
    """include/bfsm.h: a member of a batch is bitwise the single evaluation on the same handle."""
    import bfsm
    torch = torch_cuda
    fs = np.stack([_field(case, 2), 0.3 + _field(case, 3) ** 2])
    op = _op(bfsm, case, prec, max_batch=2)
    fb = torch.from_numpy(fs).cuda()
    Qb = torch.empty_like(fb)
    torch.cuda.synchronize()
    op.collideBatchPartial(Qb, fb, 2, True)
    op.synchronize()
    ones = [_partial(torch, op, fb[i]) for i in range(2)]
    op.destroy()
    for i in range(2):
        err = _rel(Qb[i].cpu().numpy(), _oracle(oracle, case, fs[i]))
        print(f"{case.name} fp{prec} member {i}: rel err {err:.2e}")
        assert torch.equal(Qb[i], ones[i]), (case.name, prec, i)
        assert err <= TOL[prec]


@pytest.mark.parametrize("case,prec", MORE_PRECS)
def test_bilinear_form_and_split(torch_cuda, case, prec):
    """Q(g,f), and Qgain / nu of Q(f,f), of the entry's directions with a rule without antipodal symmetry."""
    import bfsm
    torch = torch_cuda
    rng = np.random.default_rng(sum(case.shape) + 7)
    g_h, f_h = rng.random(case.shape) + 0.1, rng.random(case.shape) + 0.1
    sph = BR.random_rule(case.n_sph, seed=sum(case.shape))
    gl = _gl(bfsm, case)
    glq = (gl.getNodes(), gl.getWeights())
    dir_range = case.dir_range if case.dir_range != CC.ALL else None
    op = _op(bfsm, case, prec, sph=_Rule(*sph))
    g, f = torch.from_numpy(g_h).cuda(), torch.from_numpy(f_h).cuda()
    Q, Qg, nu = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    torch.cuda.synchronize()
    if dir_range:
        op.collideBilinearPartial(Q, g, f, True)
        op.collideSplitBatchPartial(Qg, nu, f, 1, True)
        op.synchronize()
    else:
        op.computeBilinearCollision(Q, g, f)
        op.computeCollisionSplit(Qg, nu, f)
    op.destroy()
    Q_ref = BR.collide_bilinear(g_h, f_h, glq, sph, GAMMA, B_GAMMA, L_BOX, dir_range=dir_range)
    Qg_ref, nu_ref = SR.split(f_h, f_h, glq, sph, GAMMA, B_GAMMA, L_BOX, dir_range=dir_range)
    errs = (_rel(Q.cpu().numpy(), Q_ref), _rel(Qg.cpu().numpy(), Qg_ref), _rel(nu.cpu().numpy(), nu_ref))
    print(f"{case.name} fp{prec}: Q(g,f) rel err {errs[0]:.2e}, Qgain {errs[1]:.2e}, nu {errs[2]:.2e}")
    assert max(errs) <= TOL[prec]
