"""Case table of the symmetric form Qs(g,f) = Q(g,f) + Q(f,g) (include/bfsm.h, bfsm_collide_symmetric*): the handles the GPU
suite runs it on, each with the plan it must take and the geometry of the phase-multiply kernel KA (csrc/bfsm_core.hpp,
body_gain_inv with GainInvBiParams) of its mode.

Plain data, importable without a GPU.  tests/test_emu_symmetric.py checks the table on the CPU (every fused cube in both
precisions has a Hermitian case; every case takes the plan it declares under the library's own make_plan; every antipodal
case can tell the operator from a single merged pass); tests/test_gpu_symmetric.py runs every entry on the GPU against
tests/symmetric_ref.py.

Modes: "hermitian" = BFSM_FLAG_EXACT_REDUCTIONS | BFSM_FLAG_HERMITIAN, "exact" = BFSM_FLAG_EXACT_REDUCTIONS, "faithful" = no
flag.  The rule of a case is symmetric_ref.antipodal_rule(n_sph / 2, seed=n): on the exact modes make_plan merges it to
sph_eff = n_sph / 2 directions of doubled weight; the faithful mode and the size-generic path evaluate all n_sph.

KA of the symmetric call (two launches per chunk, the spectra exchanged):
  groups    KA's direction groups (Pipeline::gain_spectra, groups_a = target_workgroups / a_planes x rounds, a_planes = N / 2 + 1
            on Hermitian handles, N otherwise); n_gl * sph_eff exceeds it wherever 5 radial nodes x 7 effective directions can
            (the sizes of tests/bilinear_cases.py), so that KA's workgroups loop over two or more directions; "loop" says so
  ka        the kernel kind and geometry: GainInv (body_gain_inv / body_gain_inv_pair at N = 32) with planes = a_planes;
            GainInvNyq at N = 64 on Hermitian handles (KN's workgroups, reading their spectrum by sign, as guests);
            GainInvTwo at N = 128 fp32 on Hermitian handles (two arrays on the interleaved-pairs geometry); elsewhere on
            Hermitian handles KN (NyqRowsBiParams) is a launch of its own
  No (N, precision) falls back to storing all N planes: no Hermitian bilinear KA geometry spills where its Q(g,f) form on all
  planes does not (tools/kernel_resources.py --scratch; N = 128 fp64 is the Q(g,f) instantiation itself, planes is a run-time
  parameter there).
slabs: the segments of the plan; the symmetric call writes and reduces 2 x slabs.
"""
from collections import namedtuple

EXACT, HERMITIAN = 2, 4                              # include/bfsm.h
MODES = {"faithful": 0, "exact": EXACT, "hermitian": EXACT | HERMITIAN}

# shape: N (a fused cube) or (nx, ny, nz) (a size-generic box); sph_eff, chunks, slabs: what make_plan must decide (fused cubes)
Case = namedtuple("Case", "shape prec mode n_gl n_sph sph_eff chunks slabs groups loop ka")

CASES = [
    # every fused cube x both precisions, exact + Hermitian
    Case(16, 64, "hermitian", 5, 14, 7, 1, 35, 113, False, "GainInv, planes 9; KN own launch"),
    Case(16, 32, "hermitian", 5, 14, 7, 1, 35, 113, False, "GainInv, planes 9; KN own launch"),
    Case(24, 64, "hermitian", 4, 10, 5, 1, 20, 78, False, "GainInv pair, planes 13; KN own launch"),
    Case(24, 32, "hermitian", 4, 10, 5, 1, 20, 78, False, "GainInv pair, planes 13; KN own launch"),
    Case(32, 64, "hermitian", 5, 14, 7, 1, 35, 120, False, "GainInv 32 x 64 panel, planes 17; KN own launch"),
    Case(32, 32, "hermitian", 5, 14, 7, 1, 35, 120, False, "GainInv 32 x 64 panel, planes 17; KN own launch"),
    Case(40, 64, "hermitian", 2, 14, 7, 1, 14, 48, False, "GainInv pair, re-read, planes 21; KN own launch"),
    Case(40, 32, "hermitian", 2, 14, 7, 1, 14, 48, False, "GainInv pair, planes 21; KN own launch"),
    Case(48, 64, "hermitian", 2, 12, 6, 1, 12, 40, False, "GainInv sequential, planes 25; KN own launch"),
    Case(48, 32, "hermitian", 2, 12, 6, 1, 12, 40, False, "GainInv pair, planes 25; KN own launch"),
    Case(64, 64, "hermitian", 5, 14, 7, 1, 35, 30, True, "GainInvNyq: pair KA, planes 33, + guest KN by sign"),      # cfg3's geometry
    Case(64, 32, "hermitian", 5, 14, 7, 1, 35, 30, True, "GainInvNyq: sequential KA, planes 33, + guest KN by sign"),
    Case(80, 64, "hermitian", 2, 14, 7, 1, 12, 12, True, "GainInv sequential, re-read, planes 41; KN own launch"),
    Case(80, 32, "hermitian", 2, 14, 7, 1, 8, 12, True, "GainInv sequential, re-read, planes 41; KN own launch"),
    Case(96, 64, "hermitian", 2, 12, 6, 1, 8, 10, True, "GainInv pair, re-read, planes 49; KN own launch"),
    Case(96, 32, "hermitian", 2, 12, 6, 1, 10, 10, True, "GainInv pair, planes 49; KN own launch"),
    Case(128, 64, "hermitian", 2, 8, 4, 1, 4, 7, True, "GainInv sequential, re-read, split, planes 65; KN own launch"),
    Case(128, 32, "hermitian", 2, 8, 4, 1, 4, 7, True, "GainInvTwo: pair KA storing two arrays, planes 65; KN own launch"),   # cfg5's
    # exact, all planes
    Case(16, 64, "exact", 5, 14, 7, 1, 35, 64, False, "GainInv, planes 16"),
    Case(32, 64, "exact", 5, 14, 7, 1, 35, 64, False, "GainInv 32 x 64 panel, planes 32"),
    Case(64, 64, "exact", 5, 8, 4, 1, 20, 16, True, "GainInv pair, planes 64"),
    Case(128, 32, "exact", 2, 6, 3, 1, 4, 4, True, "GainInv pair, interleaved pairs, planes 128"),
    # faithful: every direction of the rule, twice
    Case(16, 64, "faithful", 5, 14, 14, 1, 65, 64, True, "GainInv, planes 16"),
    Case(32, 64, "faithful", 5, 14, 14, 1, 35, 64, True, "GainInv 32 x 64 panel, planes 32"),
    Case(64, 64, "faithful", 2, 10, 10, 1, 8, 16, True, "GainInv pair, planes 64"),
    # size-generic boxes (the flags have no effect there)
    Case((12, 8, 20), 64, "faithful", 2, 6, 6, 1, 0, 0, False, "size-generic: bilinear plane kernels, two passes"),
    Case((20, 20, 20), 64, "faithful", 2, 6, 6, 1, 0, 0, False, "size-generic: bilinear plane kernels, two passes"),
]

# Launch-sequence variants in the exact + Hermitian mode, on the inputs of the Hermitian case of their (N, precision):
#   chunks  max_chunk = 2 (3 at N = 128): chunks that cross radial nodes, 2 x slabs > 8: the separate Reduce launch
#   single  a shard of few directions in one chunk with 2 x slabs <= 8: the reduce fused into the tail
#           (Pipeline::fuse_reduce_symmetric)
#   batch   a handle created with max_batch = 3 running the single call (the reduce route its slabs give)
# shard: full directions (None: all); chunks / slabs: what make_plan must decide; reduce: kernel_launches[BFSM_K_REDUCE]
Variant = namedtuple("Variant", "kind n prec shard max_chunk max_batch chunks slabs reduce")
VARIANT_SIZES = ((64, 64), (128, 32))
MAX_BATCH = 3
FUSE_LIMIT = 8                                       # Pipeline::fuse_reduce_symmetric: 2 * slab_count <= 8
VARIANTS = [
    Variant("chunks", 64, 64, None, 2, 0, 18, 35, 1), Variant("single", 64, 64, (0, 8), 0, 0, 1, 4, 0),
    Variant("batch", 64, 64, None, 0, MAX_BATCH, 1, 35, 1),
    Variant("chunks", 128, 32, None, 3, 0, 3, 8, 1), Variant("single", 128, 32, (0, 8), 0, 0, 1, 4, 0),
    Variant("batch", 128, 32, None, 0, MAX_BATCH, 1, 4, 0),
]


def case(shape, prec, mode):
    (c,) = [c for c in CASES if (c.shape, c.prec, c.mode) == (shape, prec, mode)]
    return c


def cid(c):
    s = f"N{c.shape}" if isinstance(c.shape, int) else "x".join(str(v) for v in c.shape)
    return f"{s}-fp{c.prec}-{c.mode}"
