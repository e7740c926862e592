"""The load-ahead direction loop of the x-line kernel (kb_sum_segment_ahead in csrc/bfsm_core.hpp; N = 64 in double
precision) through the host emulator, which compiles the same kernel body: segments of one direction (the loop does not
run), of two (one trip) and of three (two trips) against the oracle at the suite's fp64 bound -- the CPU twin of
test_gpu_line_loadahead.py::test_trip_counts, and the place where the segment lengths of its cases are asserted."""
import numpy as np
import pytest

import emu_lib

TOL64 = 1e-12
NV, N_GL = 64, 2


@pytest.mark.parametrize("n_sph,max_chunk,chunk_dirs,seg_lens", [(12, 0, [24], [3] * 8), (12, 7, [6] * 4, [1] * 24),
                                                                 (12, 4, [4] * 6, [1] * 24), (6, 0, [12], [1, 2] * 4)])
def test_plans_of_the_gpu_cases(n_sph, max_chunk, chunk_dirs, seg_lens):
    chunks, segs = emu_lib.plan(NV, N_GL, n_sph, 64, max_chunk=max_chunk)
    assert [c[2] for c in chunks] == chunk_dirs
    assert [s[2] for s in segs] == seg_lens


@pytest.mark.parametrize("n_sph,lens", [(6, {1, 2}), (12, {3})], ids=["segments-of-1-and-2", "segments-of-3"])
def test_trip_counts_match_the_oracle(oracle, n_sph, lens):
    import bfsm
    c = bfsm.reference_constants()
    _, segs = emu_lib.plan(NV, N_GL, n_sph, 64)
    assert set(s[2] for s in segs) == lens
    f = bfsm.perturbed_input(bfsm.bkw_solution(NV)[0])
    gl, sph = oracle.gauss_legendre(N_GL, 0.0, c["R"]), oracle.spherical_design(n_sph)
    ref = oracle.collide(f, gl, sph, c["gamma"], c["b_gamma"], c["L"])
    got, _ = emu_lib.collide(f, gl, sph, c["gamma"], c["b_gamma"], c["L"])
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"N=64 2x{n_sph} through the emulator, segments of {sorted(lens)}: max rel err {err:.2e}")
    assert err <= TOL64
