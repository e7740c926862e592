"""-m gpu: the batched two-operand forms (include/bfsm.h, bfsm_collide_symmetric_batch*, bfsm_collide_bilinear_batch_partial_async)
on the MI355X.

Every entry of tests/symmetric_batch_cases.py against tests/symmetric_ref.py per member on the full rule, member i bit for bit the
single call on the same handle, a shared operand bit for bit the replicated one; uneven direction shards, BFSM_FLAG_CONSERVE per
member, graph replay, independence of the handle's call history, argument errors, the profiled launch counts and the C++ mirror.
Bounds as in tests/test_gpu_bilinear.py: fp64 1e-12, fp32 5e-6, relative to max|reference|.  Every case prints its measured error.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bilinear_cases as BC
import conserve_ref as CR
import symmetric_batch_cases as SB
from test_emu_symmetric import L_BOX, TOL64, _rel, _tol
from test_emu_symmetric_batch import assert_teeth, batch_inputs, case_ref, member_ref, operands
from test_gpu_bilinear import _dev, torch_cuda  # noqa: F401
from test_gpu_symmetric import _make

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _handle(c, **kw):
    inp = batch_inputs(c)
    kw.setdefault("shard", c.shard)
    return _make(c.shape, c.prec, c.mode, inp["gl"], inp["sph"], max_chunk=c.max_chunk, max_batch=c.max_batch, **kw)


def _batch(torch, op, g, f, n_batch, share, with_loss=True, symmetric=True):
    """The batched call on NaN-filled Q; returns the device tensor [n_batch][shape]."""
    Q = torch.full((n_batch,) + tuple(g.shape[-3:]), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if symmetric:
        op.collideSymmetricBatchPartial(Q, g, f, n_batch, with_loss, share)
    else:
        op.collideBilinearBatchPartial(Q, g, f, n_batch, with_loss, share)
    op.synchronize()
    return Q


def _member(t, share_this, i):
    return t if share_this else t[i]


@pytest.mark.parametrize("c", SB.CASES, ids=SB.cid)
def test_case_matches_reference_and_the_single_call(torch_cuda, c):
    torch = torch_cuda
    assert_teeth(c)                                      # on the reference alone, before any device result
    tol = _tol(c.prec)
    gh, fh = operands(c)
    g, f = _dev(torch, gh), _dev(torch, fh)
    op = _handle(c)
    Q = _batch(torch, op, g, f, c.n_batch, c.share)
    got = Q.cpu().numpy()
    for i in range(c.n_batch):
        err = _rel(got[i], case_ref(c, i))
        print(f"{SB.cid(c)} member {i}: Qs max rel err {err:.2e} (bound {tol:.0e})")
        assert err <= tol
    one = torch.empty_like(Q[0])
    for i in range(c.n_batch):                           # bitwise the single call on the same handle
        one.fill_(float("nan"))
        op.collideSymmetricPartial(one, _member(g, c.share == "g", i), _member(f, c.share == "f", i), True)
        op.synchronize()
        assert torch.equal(one, Q[i]), (SB.cid(c), i)
    if c.share and c.n_batch >= 2:                       # bitwise the replicated operand
        gr = g.expand(c.n_batch, *g.shape).contiguous() if c.share == "g" else g
        fr = f.expand(c.n_batch, *f.shape).contiguous() if c.share == "f" else f
        assert torch.equal(_batch(torch, op, gr, fr, c.n_batch, None), Q), SB.cid(c)
    if c.mode == "faithful" and c.shard is None:         # the bilinear batch on the same handle
        B = _batch(torch, op, g, f, c.n_batch, c.share, symmetric=False)
        gotb = B.cpu().numpy()
        for i in range(c.n_batch):
            err = _rel(gotb[i], member_ref(c, i, c.share, symmetric=False))
            print(f"{SB.cid(c)} member {i}: Q(g,f) max rel err {err:.2e} (bound {tol:.0e})")
            assert err <= tol
            op.collideBilinearPartial(one, _member(g, c.share == "g", i), _member(f, c.share == "f", i), True)
            op.synchronize()
            assert torch.equal(one, B[i]), (SB.cid(c), i)
    op.destroy()


def _case(shape, prec, mode, n_batch):
    return [c for c in SB.CASES if (c.shape, c.prec, c.mode, c.n_batch) == (shape, prec, mode, n_batch) and not c.max_chunk and not c.shard][0]


def test_three_uneven_shards_sum_to_the_reference(torch_cuda):
    torch = torch_cuda
    c = _case(24, 64, "hermitian", 2)
    gh, fh = operands(c)
    g, f = _dev(torch, gh), _dev(torch, fh)
    total = np.zeros((c.n_batch,) + gh.shape[-3:])
    for rank, rng in enumerate(BC.shards(c.n_gl * c.n_sph)):
        op = _handle(c, shard=rng)
        total += _batch(torch, op, g, f, c.n_batch, c.share, with_loss=(rank == 1)).cpu().numpy()
        op.destroy()
    for i in range(c.n_batch):
        err = _rel(total[i], case_ref(c, i))
        print(f"{SB.cid(c)}: shards {BC.shards(c.n_gl * c.n_sph)} summed, member {i} max rel err {err:.2e}")
        assert err <= TOL64


@pytest.mark.parametrize("shape,prec,mode", [(24, 64, "hermitian"), (24, 32, "hermitian"), ((12, 8, 20), 64, "faithful")])
def test_conserve_projects_every_member(torch_cuda, shape, prec, mode):
    """Q_i = P Qs(g_i, f_i): the five discrete invariants of every member vanish to 1e-12 of their scale
    (tests/test_gpu_conserve.py), and Q_i is conserve_ref.project of the reference."""
    torch = torch_cuda
    c = _case(shape, prec, mode, 2)
    gh, fh = operands(c)
    op = _handle(c, conserve=True)
    got = _batch(torch, op, _dev(torch, gh), _dev(torch, fh), c.n_batch, c.share).cpu().numpy()
    op.destroy()
    for i in range(c.n_batch):
        m, s = np.abs(CR.moments(got[i], L_BOX)), CR.moment_scale(got[i], L_BOX)
        print(f"{SB.cid(c)} conserve, member {i}: moments / scale {m / s}")
        assert np.all(m <= 1e-12 * s), m / s
        assert _rel(got[i], CR.project(np.asarray(case_ref(c, i)), L_BOX)) <= _tol(prec)


def test_capture_and_replay_on_one_stream(torch_cuda):
    torch = torch_cuda
    c = _case(24, 64, "hermitian", 3)
    gh, fh = operands(c)
    g, f = _dev(torch, gh), _dev(torch, fh)
    op = _handle(c)
    Qg = torch.empty((c.n_batch,) + tuple(gh.shape[-3:]), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op.computeSymmetricCollisionBatch(Qg, g, f, c.n_batch, c.share, side.cuda_stream)      # first call outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        op.computeSymmetricCollisionBatch(Qg, g, f, c.n_batch, c.share, torch.cuda.current_stream().cuda_stream)
    varied = f if c.share != "f" else g
    src = np.asarray(fh if c.share != "f" else gh)
    for scale in (1.0, -0.5):
        varied.copy_(torch.from_numpy(src * scale))
        Qg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_batch(torch, op, g, f, c.n_batch, c.share), Qg)
        for i in range(c.n_batch):
            assert _rel(Qg[i].cpu().numpy(), scale * np.asarray(case_ref(c, i))) <= TOL64
    op.destroy()


def test_another_n_batch_in_between_changes_no_bit(torch_cuda):
    torch = torch_cuda
    c = _case(24, 64, "hermitian", 3)
    inp = batch_inputs(c)
    g, f = _dev(torch, inp["g"]), _dev(torch, inp["f"])
    for mode in ("faithful", "hermitian"):
        op = _make(24, 64, mode, inp["gl"], inp["sph"], max_batch=3)
        first = _batch(torch, op, g, f, 3, None)
        _batch(torch, op, g[0], f[:2], 2, "g")
        again = _batch(torch, op, g, f, 3, None)
        assert torch.equal(first, again), mode
        two = _batch(torch, op, g[:2], f[:2], 2, None)
        assert torch.equal(two, first[:2]), mode         # a member does not depend on n_batch
        q0, q1 = torch.empty_like(f[0]), torch.empty_like(f[0])
        op.computeCollision(q0, f[0])
        _batch(torch, op, g, f[0], 3, "f")
        op.computeCollision(q1, f[0])
        assert torch.equal(q0, q1), mode
        op.destroy()


def test_argument_errors(torch_cuda):
    torch = torch_cuda
    c = _case(24, 64, "hermitian", 3)
    inp = batch_inputs(c)
    G = 24 ** 3
    op = _make(24, 64, "hermitian", inp["gl"], inp["sph"], max_batch=3)
    part = _make(24, 64, "hermitian", inp["gl"], inp["sph"], max_batch=3, shard=(0, 8))
    lib = op._lib
    buf = torch.zeros(9 * G, dtype=torch.float64, device="cuda")
    p = lambda off: ctypes.c_void_p(buf.data_ptr() + 8 * off)
    sym, bil = lib.bfsm_collide_symmetric_batch_partial_async, lib.bfsm_collide_bilinear_batch_partial_async
    Q, g, f = p(0), p(3 * G), p(6 * G)
    for args, needle in [((None, g, f, 3, 0), b"null"), ((Q, None, f, 3, 0), b"null"), ((Q, g, None, 3, 0), b"null"),
                         ((Q, g, f, 0, 0), b"n_batch"), ((Q, g, f, 4, 0), b"n_batch"), ((Q, g, f, -1, 0), b"n_batch"),
                         ((Q, g, f, 3, 3), b"share"), ((Q, g, f, 3, -1), b"share"),
                         ((p(G), g, f, 3, 0), b"overlap"), ((Q, p(2 * G), p(6 * G), 3, 1), b"overlap"),
                         ((Q, p(0), f, 3, 0), b"overlap"), ((p(4 * G), g, p(6 * G), 2, 2), b"overlap")]:
        assert sym(op._h, *args, 1, None) == 1, args
        assert needle in lib.bfsm_last_error(op._h), lib.bfsm_last_error(op._h)
    # a shared g is G doubles: right in front of Q it does not overlap (n_batch * G doubles from there would)
    assert sym(op._h, p(4 * G), p(3 * G), p(6 * G), 2, 1, 1, None) == 0
    op.synchronize()
    buf.zero_()
    assert bil(op._h, Q, g, f, 3, 0, 1, None) == 2                     # BFSM_ERR_UNSUPPORTED on an exact handle, Q untouched
    assert lib.bfsm_collide_symmetric_batch(part._h, Q, g, f, 3, 0) == 1
    assert b"owns all directions" in lib.bfsm_last_error(part._h)
    torch.cuda.synchronize()
    assert not buf.any()
    with pytest.raises(ValueError):
        op.computeSymmetricCollisionBatch(buf[:3 * G], buf[3 * G:6 * G], buf[6 * G:], 3, share="h")
    with pytest.raises(ValueError):
        op.computeSymmetricCollisionBatch(buf[:3 * G], buf[3 * G:6 * G], buf[6 * G:], 3, share="g")     # a shared g has G elements
    gh, fh = operands(c)
    got = _batch(torch, op, _dev(torch, gh), _dev(torch, fh), c.n_batch, c.share).cpu().numpy()       # the handle still works
    assert _rel(got[2], case_ref(c, 2)) <= TOL64
    op.destroy()
    part.destroy()


@pytest.mark.parametrize("c", [c for c in SB.CASES if isinstance(c.shape, int) and c.shape == 24 and c.prec == 64 and c.mode == "hermitian"
                               and c.n_batch == 2], ids=SB.cid)
def test_profiled_launches_are_the_sequence(torch_cuda, c):
    """kernel_launches under BFSM_FLAG_PROFILE: per chunk two KA and (N = 24: KN as a launch of its own, booked under gain_inv) two
    KN and two x-line launches, then one KC, the reduce the slabs ask for, two tail kernels, two launches per input transform pass --
    whatever n_batch; the same counts as the single call."""
    from bfsm import capi
    torch = torch_cuda
    gh, fh = operands(c)
    g, f = _dev(torch, gh), _dev(torch, fh)
    op = _handle(c, profile=True)
    _batch(torch, op, g, f, c.n_batch, c.share)
    cnt = op.counters()
    batch = dict(zip(capi.KERNEL_NAMES, cnt.kernel_launches))
    one = torch.empty_like(g[0] if g.dim() == 4 else g)
    op.collideSymmetricPartial(one, _member(g, c.share == "g", 0), _member(f, c.share == "f", 0), True)
    op.synchronize()
    single = dict(zip(capi.KERNEL_NAMES, op.counters().kernel_launches))
    op.destroy()
    print(f"{SB.cid(c)}: {cnt.n_chunks} chunks, launches {batch}")
    assert cnt.n_chunks == c.chunks
    assert batch == dict(fft_f=4, gain_inv=4 * c.chunks, gain_line=2 * c.chunks, gain_fwd=1, reduce=c.reduce, tail=2)
    assert batch == single


def test_cpp_mirror(torch_cuda, tmp_path):
    """tests/host/test_symmetric_batch_mirror.cpp: the three batched calls of BoltzmannOperator<HIP_Backend>, every member bit for
    bit the single call."""
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "boltzmann-fourier-spectral-method_amd")
    exe = str(tmp_path / "test_symmetric_batch_mirror")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I", os.path.join(pkg, "host"), "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "test_symmetric_batch_mirror.cpp"),
                           os.path.join(pkg, "host", "HIPBoltzmannOperator.cpp"), os.path.join(pkg, "host", "Quadratures", "SphericalDesign.cpp"),
                           "-L" + pkg, "-lbfsm_hip", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.run([exe, os.path.join(pkg, "data", "sph_design")], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "symmetric batch mirror checks passed" in out.stdout
