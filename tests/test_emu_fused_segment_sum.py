"""The faithful mode's x-line kernel with the segment sum fused in (body_gain_line_acc on GainLineSumParams) through the
host emulator: N = 24 with 3 x 32 directions and max_chunk = 50 -- two chunks of 48 that cut the middle radial node,
segments of one and of two directions, the forward tile pass once over the segment sums of both chunks -- against the
oracle at the suite's fp64 bound."""
import numpy as np

import emu_lib

TOL64 = 1e-12
NV, N_GL, N_SPH, MAX_CHUNK = 24, 3, 32, 50


def test_plan_has_multi_direction_segments_and_a_cut_node():
    chunks, segs = emu_lib.plan(NV, N_GL, N_SPH, 64, max_chunk=MAX_CHUNK)
    assert [c[2] for c in chunks] == [48, 48]                  # 1.5 radial nodes each
    assert sorted(set(s[2] for s in segs)) == [1, 2]
    assert [s[3] for s in segs if s[0] == 0][-1] == 1 and [s[3] for s in segs if s[0] == 1][0] == 1   # node 1 is cut


def test_two_chunks_match_the_oracle(oracle):
    import bfsm
    c = bfsm.reference_constants()
    f = bfsm.perturbed_input(bfsm.bkw_solution(NV)[0])
    gl, sph = oracle.gauss_legendre(N_GL, 0.0, c["R"]), oracle.spherical_design(N_SPH)
    ref = oracle.collide(f, gl, sph, c["gamma"], c["b_gamma"], c["L"])
    got, _ = emu_lib.collide(f, gl, sph, c["gamma"], c["b_gamma"], c["L"], max_chunk=MAX_CHUNK)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"N=24 3x32 max_chunk=50 through the emulator: max rel err {err:.2e}")
    assert err <= TOL64
