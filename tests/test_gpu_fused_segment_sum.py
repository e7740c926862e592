"""-m gpu: the faithful mode's x-line kernel with the segment sum fused in (body_gain_line_acc on GainLineSumParams): P' of a
direction never reaches memory, the kernel writes one sum per segment and ONE forward tile pass over the sums follows all
chunks.

What the rest of the suite does not pin down: segments of several directions in one and in several chunks, chunks that cut
a radial node, shards that start inside a node, of one direction and of none, the batch stride of the segment sums on the
interleaved-pair geometry, no state carried from one evaluation to the next, and the launch accounting that shows P' is gone.
Inputs and bounds are the suite's: the perturbed input of test_gpu_parity._full_ref, 1e-12 max|Q| in fp64, 5e-6 in fp32, both
against the oracle.  Every case prints its measured error."""
import numpy as np
import pytest

from test_gpu_parity import TOL32, TOL64, _collide, _full_ref, _make, _oracle, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

# geometries DESIGN.md 7.5 leaves on the per-direction route (body_gain_line + one KC per chunk): (N, precision)
PER_DIRECTION_ROUTE = ((80, 64), (80, 32), (96, 64), (96, 32), (128, 64))


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _input(nv):
    import bfsm
    return bfsm.perturbed_input(bfsm.bkw_solution(nv)[0])


def _partial(torch, op, f_h):
    f = torch.from_numpy(np.ascontiguousarray(f_h)).cuda()
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.collidePartial(Q, f, with_loss=True)
    op.synchronize()
    return Q.cpu().numpy()


# Segments of make_plan at N = 64 (8 workgroup columns per x-plane wanted): 2 x 12 directions in one chunk are 2 radial runs
# cut 4 ways = 8 segments of 3; max_chunk = 7 gives 4 chunks of 6 directions, half a node each, cut into 6 segments of 1
# (a run is never cut into more segments than it has directions) = 24; config 3 (16 x 48) is 16 runs, one segment each.
@pytest.mark.parametrize("max_chunk,chunks,n_seg", [(0, 1, 8), (7, 4, 24)], ids=["whole", "chunk7"])
def test_segments_of_three_directions(torch_cuda, oracle, max_chunk, chunks, n_seg):
    """N = 64 fp64, 2 x 12 directions: one chunk gives 8 segments of 3 directions; max_chunk = 7 gives 4 chunks of 6 that cut
    both radial nodes, and the forward tile pass runs once over the segments of all chunks (its marked bytes count them)."""
    import bfsm
    from bfsm import capi
    nv, n_gl, n_sph = 64, 2, 12
    f_h, ref = _full_ref(oracle, nv, n_gl, n_sph)
    op = _make(bfsm, nv, n_gl, n_sph, 64, max_chunk=max_chunk, profile=True)
    got = _collide(torch_cuda, op, f_h)
    cnt = op.counters()
    op.destroy()
    launches = tuple(cnt.kernel_launches)
    err = _rel(got, ref)
    segments = cnt.kernel_alg_bytes[capi.KERNEL_NAMES.index("gain_fwd")] / (float(nv) ** 3 * 16.0)
    print(f"N=64 fp64 2x12 max_chunk={max_chunk}: {cnt.n_chunks} chunks, {segments:.0f} segments, launches {launches}, max rel err {err:.2e}")
    assert cnt.n_chunks == chunks
    assert segments == n_seg
    assert launches[capi.KERNEL_NAMES.index("gain_line")] == chunks
    assert launches[capi.KERNEL_NAMES.index("gain_fwd")] == 1
    assert err <= TOL64


@pytest.mark.parametrize("shard", [(5, 19), (13, 14), (7, 7)], ids=["mid-node", "one-direction", "empty"])
def test_shards(torch_cuda, oracle, shard):
    """A shard that starts and ends inside a radial node, a shard of one direction (a segment of one) and an empty shard
    (no gain launch at all: Q = -loss), each against the oracle's gain over the same directions."""
    import bfsm
    nv, n_gl, n_sph = 64, 2, 12
    f_h = _input(nv)
    ref = _oracle(oracle, f_h, n_gl, n_sph, dir_range=shard)
    op = _make(bfsm, nv, n_gl, n_sph, 64, shard=shard)
    got = _partial(torch_cuda, op, f_h)
    op.destroy()
    err = _rel(got, ref)
    print(f"N=64 fp64 2x12 shard {shard}: max rel err {err:.2e}")
    assert err <= TOL64


def test_whole_wave_row_geometry(torch_cuda, oracle):
    """N = 32 fp64, 5 x 14 directions (a 14-point rule without antipodal symmetry): two rows of the inner space per
    workgroup, so that a row of threads is a whole wave; 5 radial runs cut 7 ways: segments of two directions."""
    import bfsm
    import bilinear_ref as BR
    from test_gpu_bilinear import _Rule
    nv, n_gl, n_sph = 32, 5, 14
    c = bfsm.reference_constants()
    f_h = _input(nv)
    gl = bfsm.GaussLegendreQuadrature(n_gl, 0.0, c["R"])
    sph = BR.random_rule(n_sph, seed=nv)
    ref = oracle.collide(f_h, (gl.getNodes(), gl.getWeights()), sph, c["gamma"], c["b_gamma"], c["L"])
    op = bfsm.HIPBoltzmannOperator(gl, _Rule(*sph), nv, nv, nv, c["gamma"], c["b_gamma"], c["L"])
    op.setProfiling(True)
    op.initialize()
    got = _collide(torch_cuda, op, f_h)
    segments = op.counters().kernel_alg_bytes[3] / (float(nv) ** 3 * 16.0)     # gain_fwd: one array per segment
    op.destroy()
    err = _rel(got, ref)
    print(f"N=32 fp64 5x14: {segments:.0f} segments, max rel err {err:.2e}")
    assert segments == 35
    assert err <= TOL64


def test_interleaved_pairs_with_a_batch(torch_cuda, oracle):
    """N = 128 fp32, 2 x 12 directions on a handle created for batches of two: the pair loads of the loop and the batch
    stride of the segment sums (member 1 is a different field; each member against its own oracle field)."""
    import bfsm
    torch = torch_cuda
    nv, n_gl, n_sph = 128, 2, 12
    f0, ref0 = _full_ref(oracle, nv, n_gl, n_sph)
    f1 = np.ascontiguousarray(f0[::-1, :, :] * 1.25)
    ref1 = _oracle(oracle, f1, n_gl, n_sph)
    op = _make(bfsm, nv, n_gl, n_sph, 32, max_batch=2)
    f = torch.from_numpy(np.stack([f0, f1])).cuda()
    Q = torch.empty_like(f)
    torch.cuda.synchronize()
    op.computeCollisionBatch(Q, f, 2)
    got = Q.cpu().numpy()
    op.destroy()
    e0, e1 = _rel(got[0], ref0), _rel(got[1], ref1)
    print(f"N=128 fp32 2x12 batch of 2: max rel err {e0:.2e}, {e1:.2e}")
    assert e0 <= TOL32 and e1 <= TOL32


def test_no_stale_state(torch_cuda):
    """Two different inputs back to back on one handle: each equals its own fresh-handle result bitwise (the accumulators
    start from zero, the segment sums are overwritten)."""
    import bfsm
    nv, n_gl, n_sph = 64, 2, 12
    fa = _input(nv)
    fb = np.ascontiguousarray(fa.transpose(2, 0, 1) * 0.5 + 0.25 * fa)
    op = _make(bfsm, nv, n_gl, n_sph, 64)
    a1 = _collide(torch_cuda, op, fa)
    b1 = _collide(torch_cuda, op, fb)
    a2 = _collide(torch_cuda, op, fa)
    op.destroy()
    fresh = {}
    for k, f_h in (("a", fa), ("b", fb)):
        o = _make(bfsm, nv, n_gl, n_sph, 64)
        fresh[k] = _collide(torch_cuda, o, f_h)
        o.destroy()
    assert not np.array_equal(fresh["a"], fresh["b"])
    assert np.array_equal(a1, fresh["a"]) and np.array_equal(b1, fresh["b"]) and np.array_equal(a2, fresh["a"])


@pytest.mark.parametrize("n_gl,n_sph,max_chunk,n_seg", [(16, 48, 0, 16), (2, 12, 7, 24)], ids=["cfg3", "2x12-chunk7"])
def test_p_prime_is_gone(torch_cuda, n_gl, n_sph, max_chunk, n_seg):
    """Launch accounting of a profiled N = 64 handle: the line kernel reads two arrays per direction and writes one per
    segment, the forward tile pass reads one array per segment."""
    import bfsm
    from bfsm import capi
    nv, prec = 64, 64
    if (nv, prec) in PER_DIRECTION_ROUTE:
        pytest.skip("geometry left on the per-direction route (DESIGN.md 7.5)")
    n = n_gl * n_sph
    Gc = float(nv) ** 3 * 16.0
    op = _make(bfsm, nv, n_gl, n_sph, prec, max_chunk=max_chunk, profile=True)
    _collide(torch_cuda, op, _input(nv))
    cnt = op.counters()
    op.destroy()
    line = cnt.kernel_alg_bytes[capi.KERNEL_NAMES.index("gain_line")]
    fwd = cnt.kernel_alg_bytes[capi.KERNEL_NAMES.index("gain_fwd")]
    print(f"N=64 fp64 {n_gl}x{n_sph} max_chunk={max_chunk}: n={n} segments={n_seg} gain_line {line / Gc:.1f} Gc, gain_fwd {fwd / Gc:.1f} Gc, "
          f"moved {cnt.moved_bytes_per_eval / Gc:.1f} Gc")
    assert cnt.exact_reductions == 0
    assert line == (2 * n + n_seg) * Gc
    assert fwd == n_seg * Gc
    assert cnt.moved_bytes_per_eval == (4 * n + 4 * n_seg + 9) * Gc
