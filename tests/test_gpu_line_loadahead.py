"""-m gpu: the load-ahead schedule of the looping x-line kernel (kb_loads_ahead / kb_sum_segment_ahead in csrc/bfsm_core.hpp;
N = 64 in double precision).  The loop requests the next direction's rows while the current one is transformed; the last
direction of a segment runs behind the loop without a request.  What can go wrong is the trip count and the last request:
segments of three, two and one directions (two trips, one trip, none), shards whose last direction is the last one of the
scratch (a request past it would read outside the shard), the batch stride of the early requests, and state carried from
one evaluation to the next.

Inputs and bounds are the suite's: the perturbed input of test_gpu_parity._full_ref, 1e-12 max|Q| in fp64 against the oracle.
Every case prints its measured error."""
import numpy as np
import pytest

from test_gpu_parity import TOL64, _collide, _full_ref, _make, _oracle, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

NV, N_GL, N_SPH = 64, 2, 12
_SHARD_REF = {}


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _input(nv):
    import bfsm
    return bfsm.perturbed_input(bfsm.bkw_solution(nv)[0])


def _shard_ref(oracle, shard):
    if shard not in _SHARD_REF:
        _SHARD_REF[shard] = _oracle(oracle, _input(NV), N_GL, N_SPH, dir_range=shard)
    return _SHARD_REF[shard]


# Segments of make_plan at N = 64 (test_gpu_fused_segment_sum.py has the planner's arithmetic; tests/emu_lib.plan gives the
# same rows on the CPU): 2 x 12 directions in one chunk = 8 segments of 3; max_chunk = 7 -> 4 chunks of 6 = 24 segments of
# 1; max_chunk = 4 -> 6 chunks of 4, which the planner also cuts into 24 segments of 1 (a chunk is cut 4 ways); 2 x 6
# directions in one chunk = 8 segments of 1, 2, 1, 2, ...: the segments of 2.
@pytest.mark.parametrize("n_sph,max_chunk,chunks,seg_lens", [(12, 0, 1, [3] * 8), (12, 7, 4, [1] * 24), (12, 4, 6, [1] * 24),
                                                             (6, 0, 1, [1, 2] * 4)],
                         ids=["segments-of-3", "chunk7-segments-of-1", "chunk4", "segments-of-1-and-2"])
def test_trip_counts(torch_cuda, oracle, n_sph, max_chunk, chunks, seg_lens):
    """Three directions (two trips of the loop and the last direction behind it), one direction (the loop does not run,
    nothing is requested ahead) and two directions (one trip).  The segment count is asserted from the launch accounting;
    the lengths are the planner's (asserted on the CPU in test_emu_line_loadahead.py)."""
    import bfsm
    from bfsm import capi
    f_h, ref = _full_ref(oracle, NV, N_GL, n_sph)
    op = _make(bfsm, NV, N_GL, n_sph, 64, max_chunk=max_chunk, profile=True)
    got = _collide(torch_cuda, op, f_h)
    cnt = op.counters()
    op.destroy()
    segments = cnt.kernel_alg_bytes[capi.KERNEL_NAMES.index("gain_fwd")] / (float(NV) ** 3 * 16.0)
    err = _rel(got, ref)
    print(f"N=64 fp64 2x{n_sph} max_chunk={max_chunk}: {cnt.n_chunks} chunks, {segments:.0f} segments of {sorted(set(seg_lens))}, "
          f"max rel err {err:.2e}")
    assert cnt.n_chunks == chunks
    assert segments == len(seg_lens) and sum(seg_lens) == N_GL * n_sph
    assert err <= TOL64


@pytest.mark.parametrize("shard", [(13, 14), (5, 19), (7, 7)], ids=["one-direction", "mid-node", "empty"])
def test_shards(torch_cuda, oracle, shard):
    """A shard of a single direction (its scratch holds one direction: a request ahead would leave it), a shard that starts
    and ends inside a radial node, and an empty shard (no gain launch: Q = -loss)."""
    import bfsm
    torch = torch_cuda
    ref = _shard_ref(oracle, shard)
    op = _make(bfsm, NV, N_GL, N_SPH, 64, shard=shard)
    f = torch.from_numpy(np.ascontiguousarray(_input(NV))).cuda()
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.collidePartial(Q, f, with_loss=True)
    op.synchronize()
    got = Q.cpu().numpy()
    op.destroy()
    err = _rel(got, ref)
    print(f"N=64 fp64 2x12 shard {shard}: max rel err {err:.2e}")
    assert err <= TOL64


def test_batch_of_two_fields(torch_cuda, oracle):
    """Two different fields in one call on a max_batch = 2 handle: the requests ahead carry the member's batch stride (each
    member against its own oracle field)."""
    import bfsm
    torch = torch_cuda
    f0, ref0 = _full_ref(oracle, NV, N_GL, N_SPH)
    f1 = np.ascontiguousarray(f0[::-1, :, :] * 1.25)
    ref1 = _oracle(oracle, f1, N_GL, N_SPH)
    op = _make(bfsm, NV, N_GL, N_SPH, 64, max_batch=2)
    f = torch.from_numpy(np.stack([f0, f1])).cuda()
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.computeCollisionBatch(Q, f, 2)
    got = Q.cpu().numpy()
    op.destroy()
    e0, e1 = _rel(got[0], ref0), _rel(got[1], ref1)
    print(f"N=64 fp64 2x12 batch of 2: max rel err {e0:.2e}, {e1:.2e}")
    assert e0 <= TOL64 and e1 <= TOL64


def test_back_to_back_equals_fresh_handles(torch_cuda):
    """Two different inputs back to back on one handle: each equals its own fresh-handle result bitwise."""
    import bfsm
    fa = _input(NV)
    fb = np.ascontiguousarray(fa.transpose(2, 0, 1) * 0.5 + 0.25 * fa)
    op = _make(bfsm, NV, N_GL, N_SPH, 64)
    a1 = _collide(torch_cuda, op, fa)
    b1 = _collide(torch_cuda, op, fb)
    a2 = _collide(torch_cuda, op, fa)
    op.destroy()
    fresh = {}
    for k, f_h in (("a", fa), ("b", fb)):
        o = _make(bfsm, NV, N_GL, N_SPH, 64)
        fresh[k] = _collide(torch_cuda, o, f_h)
        o.destroy()
    assert not np.array_equal(fresh["a"], fresh["b"])
    assert np.array_equal(a1, fresh["a"]) and np.array_equal(b1, fresh["b"]) and np.array_equal(a2, fresh["a"])
