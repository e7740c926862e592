"""-m gpu: the macroscopic state of f and its Maxwellian (include/bfsm.h: bfsm_moments_async, bfsm_maxwellian_async) on the MI355X.

Parity with the numpy restatement tests/moments_ref.py at its derived tolerances on the one-launch form, the two-launch form
on a fused cube and size-generic boxes; independence of the handle's precision and direction shard; batches, determinism, graph
replay, the round trip moments(maxwellian(moments(f))), the BKW state, the argument errors and the C++ mirror.  The quadrature
is irrelevant here: every handle uses two radial nodes and the 6-point design."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import moments_ref as MR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
L_BOX = 11.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (the HIP path has no fallback)")
    return torch


def _op(shape, prec=64, shard=None, max_batch=0, L=L_BOX):
    import bfsm
    c = bfsm.reference_constants()
    op = bfsm.HIPBoltzmannOperator(bfsm.GaussLegendreQuadrature(2, 0.0, c["R"]), bfsm.SphericalDesign(6), *shape,
                                   c["gamma"], c["b_gamma"], L)
    op.setPrecision(prec)
    if shard:
        op.setDirectionShard(*shard)
    if max_batch:
        op.setMaxBatch(max_batch)
    op.initialize()
    return op


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _row(rho, u, T):
    r = np.zeros(MR.COUNT)
    r[[MR.RHO, MR.UX, MR.UY, MR.UZ, MR.T]] = rho, u[0], u[1], u[2], T
    return r


def _input(shape, seed, scale=1.0):
    """A drifting Maxwellian times a rough positive factor: every moment far from zero."""
    rng = np.random.default_rng(seed)
    return scale * MR.maxwellian(_row(1.3, (0.7, -0.4, 0.3), 2.0), shape, L_BOX) * (0.5 + rng.random(shape))


def _run(torch, op, f_h):
    """moments then maxwellian of f_h ([nx,ny,nz] or [nb,nx,ny,nz]) -> (rows, M) as numpy; f must come back unchanged."""
    nb = f_h.shape[0] if f_h.ndim == 4 else 1
    f = _dev(torch, f_h)
    mom = torch.full((nb, MR.COUNT), float("nan"), dtype=torch.float64, device="cuda")
    M = torch.full_like(f, float("nan"))
    op.moments(mom, f, nb)
    op.maxwellian(M, mom, nb)
    op.synchronize()
    assert np.array_equal(f.cpu().numpy(), f_h)
    rows = mom.cpu().numpy()
    return (rows if f_h.ndim == 4 else rows[0]), M.cpu().numpy()


# (16,16,16): G = 4096, the one-launch form; (24,24,24): Sums + Finish over four workgroups on a fused cube; (12,8,20) and
# (10,6,14): size-generic handles (one-launch form; 420 pairs are no multiple of the 256-thread stride)
@pytest.mark.parametrize("shape", [(16, 16, 16), (24, 24, 24), (12, 8, 20), (10, 6, 14)])
def test_parity_with_numpy(torch_cuda, shape):
    f_h = _input(shape, sum(shape))
    op = _op(shape)
    row, M = _run(torch_cuda, op, f_h)
    op.destroy()
    MR.assert_row(row, f_h, L_BOX, shape)
    MR.assert_maxwellian(M, row, L_BOX, shape)
    assert M.min() > 0


@pytest.mark.parametrize("shape", [(24, 24, 24), (12, 8, 20)])
def test_precision_and_shard_do_not_change_a_bit(torch_cuda, shape):
    f_h = _input(shape, 5)
    want = None
    for kw in (dict(prec=64), dict(prec=32), dict(prec=64, shard=(3, 8))):
        op = _op(shape, **kw)
        got = _run(torch_cuda, op, f_h)
        op.destroy()
        if want is None:
            want = got
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), kw


@pytest.mark.parametrize("shape", [(24, 24, 24), (16, 16, 16)])
def test_batch_members_are_bitwise_the_singles(torch_cuda, shape):
    fs = np.stack([_input(shape, 10 + i, scale=10.0 ** (3 * i - 3)) for i in range(3)])
    op = _op(shape, max_batch=4)
    rows, Ms = _run(torch_cuda, op, fs)
    for i in range(3):
        row, M = _run(torch_cuda, op, fs[i])
        assert np.array_equal(rows[i], row) and np.array_equal(Ms[i], M), i
        MR.assert_row(rows[i], fs[i], L_BOX, i)
    op.destroy()


def test_empty_and_indefinite_members_get_a_zero_maxwellian(torch_cuda):
    shape = (24, 24, 24)
    rng = np.random.default_rng(2)
    fs = np.stack([_input(shape, 1), np.zeros(shape), rng.standard_normal(shape), _input(shape, 3, 7.0)])
    op = _op(shape, max_batch=4)
    rows, Ms = _run(torch_cuda, op, fs)
    assert np.array_equal(rows[1], np.zeros(MR.COUNT)) and not Ms[1].any()
    MR.assert_row(rows[2], fs[2], L_BOX)                      # negative points: finite H, equal to the restatement
    assert np.isfinite(rows[2]).all()
    want2 = MR.maxwellian(rows[2], shape, L_BOX)              # zero unless this noise happens to have rho, T > 0
    assert np.abs(Ms[2] - want2).max() <= 64 * MR.EPS * max(want2.max(), 0.0)
    for i in (0, 3):
        row, M = _run(torch_cuda, op, fs[i])
        assert np.array_equal(rows[i], row) and np.array_equal(Ms[i], M) and M.min() > 0
    # rows a caller fills itself: rho or T not finite and positive -> M = 0, the neighbour untouched
    mom = _dev(torch_cuda, np.stack([_row(np.nan, (0, 0, 0), 1.0), _row(1.0, (0, 0, 0), -1.0), _row(np.inf, (0, 0, 0), 1.0),
                                     _row(1.3, (0.4, -0.3, 0.2), 1.5)]))
    M = torch_cuda.full((4,) + shape, float("nan"), dtype=torch_cuda.float64, device="cuda")
    op.maxwellian(M, mom, 4)
    op.synchronize()
    M = M.cpu().numpy()
    assert not M[:3].any()
    MR.assert_maxwellian(M[3], _row(1.3, (0.4, -0.3, 0.2), 1.5), L_BOX)
    op.destroy()


def test_two_runs_are_bitwise_equal(torch_cuda):
    shape = (24, 24, 24)
    f_h = _input(shape, 4)
    op = _op(shape)
    first = _run(torch_cuda, op, f_h)
    for _ in range(5):
        again = _run(torch_cuda, op, f_h)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    op.destroy()


def test_moments_then_maxwellian_replays_in_a_graph(torch_cuda):
    torch = torch_cuda
    shape = (24, 24, 24)
    f0 = _input(shape, 6)
    op = _op(shape)
    f = _dev(torch, f0)
    mom = torch.zeros(1, MR.COUNT, dtype=torch.float64, device="cuda")
    mom_g, M, M_g = torch.zeros_like(mom), torch.empty_like(f), torch.empty_like(f)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op.moments(mom_g, f, 1, side.cuda_stream)                       # first calls outside the capture
        op.maxwellian(M_g, mom_g, 1, side.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        op.moments(mom_g, f, 1, s)
        op.maxwellian(M_g, mom_g, 1, s)
    for scale in (1.0, 0.5):
        f.copy_(torch.from_numpy(f0 * scale))
        mom_g.zero_()
        M_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        op.moments(mom, f)
        op.maxwellian(M, mom)
        op.synchronize()
        assert torch.equal(mom, mom_g) and torch.equal(M, M_g)
        assert abs(mom[0, MR.RHO].item() / scale - MR.moments(f0, L_BOX)[MR.RHO]) < 1e-12
    op.destroy()


# the discrete moments of a resolved Maxwellian are its parameters up to quadrature error, which numpy alone shows to be
# 2.8e-14 at 24^3, T = 1.5 and 8.3e-11 at 16^3, T = 2.5 (L = 11)
@pytest.mark.parametrize("n,T,tol", [(24, 1.5, 1e-12), (16, 2.5, 1e-9)])
def test_round_trip_of_a_resolved_maxwellian(torch_cuda, n, T, tol):
    shape = (n, n, n)
    rho, u = 1.3, (0.4, -0.3, 0.2)
    f_h = MR.maxwellian(_row(rho, u, T), shape, 11.0)
    op = _op(shape, L=11.0)
    row1, M1 = _run(torch_cuda, op, f_h)
    row2, _ = _run(torch_cuda, op, M1)
    op.destroy()
    for row in (row1, row2):
        got = row[[MR.RHO, MR.UX, MR.UY, MR.UZ, MR.T]]
        err = np.abs(got - np.array([rho, *u, T])).max()
        print(f"round trip {n}^3: max defect {err:.3e} (bound {tol:g})")
        assert err <= tol, (got, err)


def test_bkw_state(torch_cuda):
    import bfsm
    f_h, _, L, _ = bfsm.bkw_solution(16)
    op = _op((16, 16, 16), L=L)
    row, _ = _run(torch_cuda, op, f_h)
    op.destroy()
    want = MR.assert_row(row, f_h, L, "BKW")
    assert abs(want[MR.RHO] - 1) < 0.1 and abs(want[MR.T] - 1) < 0.1 and want[MR.H] < 0      # BKW: rho = T = 1, coarsely resolved at N = 16


def test_argument_errors_leave_outputs_and_handle_alone(torch_cuda):
    torch = torch_cuda
    shape = (12, 8, 20)
    G = int(np.prod(shape))
    f_h = _input(shape, 8)
    op = _op(shape, max_batch=2)
    lib, h = op._lib, op._h
    buf = torch.zeros(2 * G + 64, dtype=torch.float64, device="cuda")      # f, then room for overlapping / misaligned views
    buf[:G] = _dev(torch, f_h).reshape(-1)
    mom = torch.full((2, MR.COUNT), 7.0, dtype=torch.float64, device="cuda")
    M = torch.full((2 * G,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 8 * off)
    assert buf.data_ptr() % 16 == 0 and M.data_ptr() % 16 == 0
    bad_moments = [
        ((None, p(buf), 1), b"null"), ((p(mom), None, 1), b"null"),
        ((p(mom), p(buf, 1), 1), b"aligned"),
        ((p(mom), p(buf), 0), b"n_batch"), ((p(mom), p(buf), 3), b"n_batch"), ((p(mom), p(buf), -1), b"n_batch"),
        ((p(buf, G - 2), p(buf), 1), b"overlap"), ((p(buf, 2 * G - 4), p(buf), 2), b"overlap"),
    ]
    for args, needle in bad_moments:
        assert lib.bfsm_moments_async(h, *args, None) == 1, args
        assert needle in lib.bfsm_last_error(h), (args, lib.bfsm_last_error(h))
    bad_maxwellian = [
        ((None, p(mom), 1), b"null"), ((p(M), None, 1), b"null"),
        ((p(M, 1), p(mom), 1), b"aligned"),
        ((p(M), p(mom), 0), b"n_batch"), ((p(M), p(mom), 3), b"n_batch"),
        ((p(M), p(M, G - 4), 1), b"overlap"), ((p(M), p(M, 2 * G - 10), 2), b"overlap"),
    ]
    for args, needle in bad_maxwellian:
        assert lib.bfsm_maxwellian_async(h, *args, None) == 1, args
        assert needle in lib.bfsm_last_error(h), (args, lib.bfsm_last_error(h))
    torch.cuda.synchronize()
    assert (mom == 7.0).all() and (M == 7.0).all() and not buf[G:].any()
    assert np.array_equal(buf[:G].cpu().numpy().reshape(shape), f_h)
    row, Mx = _run(torch, op, f_h)                                          # the handle still works
    MR.assert_row(row, f_h, L_BOX)
    MR.assert_maxwellian(Mx, row, L_BOX)
    op.destroy()


def test_cpp_mirror(torch_cuda, tmp_path):
    """tests/host/test_moments_mirror.cpp: op.moments and op.maxwellian of BoltzmannOperator<HIP_Backend> on the BKW state at
    N = 16 against host loops."""
    root = os.path.dirname(HERE)
    pkg = os.path.join(root, "boltzmann-fourier-spectral-method_amd")
    exe = str(tmp_path / "test_moments_mirror")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I", os.path.join(pkg, "host"), "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "test_moments_mirror.cpp"),
                           os.path.join(pkg, "host", "HIPBoltzmannOperator.cpp"), os.path.join(pkg, "host", "Quadratures", "SphericalDesign.cpp"),
                           "-L" + pkg, "-lbfsm_hip", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.run([exe, os.path.join(pkg, "data", "sph_design")], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "moments mirror checks passed" in out.stdout
