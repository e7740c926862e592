"""-m gpu: BFSM_FLAG_EXACT_REDUCTIONS and BFSM_FLAG_HERMITIAN on every fused cube, precision and launch-sequence variant of
tests/mode_cases.py on the MI355X.

Every variant against the oracle on the full rule (no antipodal merge, no Hermitian shortcut): several chunks with the separate
Reduce launch, few slabs with the reduce fused into the tail, three uneven direction shards (one of them empty in effective
directions) summed after collidePartial, a two-member batch on a handle created for three, and a rule without antipodal
symmetry.  Each handle must report the plan the table declares (bfsm_get_counters) and, profiled, the launches that go with
it.  N = 16 runs on the whole-direction kernels and, with BFSM_FLAG_NO_SMALL_PATH, on the plane-tile pipeline.  Bounds: fp64
1e-12, fp32 5e-6, relative to max|Q_ref| (TOL64 / TOL32 of tests/test_gpu_parity.py).  tests/test_emu_modes.py shows on the CPU
that these cases notice a missing direction (>= 1000 bounds) and the input's Nyquist planes (>= 100 bounds).  Every case prints
its measured error.
"""
import numpy as np
import pytest

import mode_cases as MC
from test_gpu_parity import TOL32, TOL64, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


class _Quad:
    """A quadrature object (the interface HIPBoltzmannOperator reads) over the oracle's arrays: (nodes, weights) of the
    radial rule, or (x, y, z, w) of the spherical one."""

    def __init__(self, *arrays):
        self.a = arrays

    def getNodes(self): return self.a[0]
    def getx(self): return self.a[0]
    def gety(self): return self.a[1]
    def getz(self): return self.a[2]
    def getWeights(self): return self.a[-1]
    def getNumberOfPoints(self): return len(self.a[-1])


def _tol(prec):
    return TOL64 if prec == 64 else TOL32


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _make(bfsm, oracle, v, part):
    op = bfsm.HIPBoltzmannOperator(_Quad(*oracle.gauss_legendre(v.n_gl, 0.0, MC.R_MAX)), _Quad(*MC.rule(oracle, v)), v.n, v.n, v.n,
                                   MC.GAMMA, MC.B_GAMMA, MC.inputs(oracle, v.n)["L"])
    op.setPrecision(v.prec)
    if part.shard:
        op.setDirectionShard(*part.shard)
    op.setMaxChunk(v.max_chunk)
    op.setMaxBatch(v.max_batch)
    op.setExactReductions(True, hermitian=(v.mode == "hermitian"))
    op.setSmallPath(v.small is not False)
    op.setProfiling(True)
    op.initialize()
    return op


def _check_plan(v, part, op):
    """The handle took the declared plan and its last call the launches that go with it."""
    from bfsm import capi
    cn = op.counters()
    got = (cn.n_chunks, cn.chunk_dirs, cn.n_dirs, cn.antipodal_merged, cn.exact_reductions)
    assert got == (part.n_chunks, part.chunk_dirs, part.n_dirs, v.merged, 1), (MC.vid(v), part, got)
    launches = tuple(cn.kernel_launches)
    gain_inv, reduce_ = MC.launches(v, part)
    assert launches[capi.KERNEL_NAMES.index("gain_inv")] == gain_inv, (MC.vid(v), part, launches)
    assert launches[capi.KERNEL_NAMES.index("reduce")] == reduce_, (MC.vid(v), part, launches)
    return launches


@pytest.mark.parametrize("v", [v for v in MC.VARIANTS if v.kind != "batch"], ids=MC.vid)
def test_variant_matches_oracle(torch_cuda, oracle, v):
    """many / noanti: the blocking call on the whole handle; few / shards: collidePartial on every shard, loss on rank 0,
    summed."""
    import bfsm
    torch = torch_cuda
    inp = MC.inputs(oracle, v.n)
    ref = MC.reference(oracle, v)
    f = torch.from_numpy(inp["f"]).cuda()
    total = np.zeros_like(inp["f"])
    seen = []
    for rank, part in enumerate(v.parts):
        op = _make(bfsm, oracle, v, part)
        Q = torch.empty_like(f)
        torch.cuda.synchronize()
        if part.shard:
            op.collidePartial(Q, f, rank == 0)
            op.synchronize()
        else:
            op(Q, f)
        total += Q.cpu().numpy()
        seen.append(_check_plan(v, part, op))
        op.destroy()
    err = _rel(total, ref)
    print(f"{MC.vid(v)}: launches {seen}, max rel err {err:.2e} (bound {_tol(v.prec):.0e})")
    assert err <= _tol(v.prec)


@pytest.mark.parametrize("v", [v for v in MC.VARIANTS if v.kind == "batch"], ids=MC.vid)
def test_batch_members_match_oracle_and_the_single_call(torch_cuda, oracle, v):
    """n_batch = 2 on a handle created for max_batch = 3, chunked: each member against its own reference, and bitwise the
    single call on the same handle."""
    import bfsm
    torch = torch_cuda
    inp = MC.inputs(oracle, v.n)
    (part,) = v.parts
    fs = torch.from_numpy(np.stack([inp["f"], inp["f1"]])).cuda()
    op = _make(bfsm, oracle, v, part)
    Qb = torch.empty_like(fs)
    torch.cuda.synchronize()
    op.computeCollisionBatch(Qb, fs, v.n_batch)
    launches = _check_plan(v, part, op)
    got = Qb.cpu().numpy()
    single = torch.empty_like(fs[0])
    for i in range(v.n_batch):
        op(single, fs[i].contiguous())
        assert np.array_equal(single.cpu().numpy(), got[i]), (MC.vid(v), i)
    _check_plan(v, part, op)
    op.destroy()
    errs = [_rel(got[i], MC.reference(oracle, v, i)) for i in range(v.n_batch)]
    print(f"{MC.vid(v)}: launches {launches}, max rel err of the members {errs[0]:.2e}, {errs[1]:.2e} (bound {_tol(v.prec):.0e})")
    assert max(errs) <= _tol(v.prec)
