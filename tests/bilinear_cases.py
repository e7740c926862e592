"""Case table of the bilinear form Q(g,f) on the fused cubes (csrc/bfsm_pipeline.hpp, fused_grid): the (N, precision) pairs
the GPU suite runs, each with the geometry of the phase-multiply kernel KA (csrc/bfsm_core.hpp, body_gain_inv with
GainInvBiParams) that it compiles to, and the launch-sequence variants of the fused bilinear path.

Plain data, importable without a GPU.  tests/test_emu_bilinear.py checks the table on the CPU: every fused cube size in both
precisions has a case, and every variant takes the plan it declares (chunks, slabs, and so the reduce route) under the
library's own make_plan.  tests/test_gpu_bilinear_cubes.py runs every entry on the GPU against tests/bilinear_ref.py.

KA's geometry is chosen at compile time (bfsm_core.hpp):
  pair      pipelined_pair: the alpha and conj(alpha) tiles of a direction go through the exchange buffer as a software-
            pipelined pair; otherwise one tile after the other ("sequential": a run-time sign loop, or at N >= 64 with the
            plane kept a compile-time sign per tile)
  keep      keep_plane: g_hat's plane (the alpha tile's operand) stays in registers across the direction loop; "re-read":
            it is re-read from L2 per direction like f_hat's plane, which the bilinear KA re-reads in every geometry
            (REREAD_BI); the bilinear form turns the kept plane off at N = 80 in single precision only
  split     split_tile: the exchange goes through a scalar buffer, real then imaginary parts (N = 128 in double precision)
  pairs-il  ab_interleaved: {A1', A2'} of a point stored side by side (N = 128 in single precision)
N = 32 has a kernel of its own (body_gain_inv_pair: both tiles side by side as one 32 x 64 panel, each half keeping its
own operand's plane).

A cube case:
  n, prec     grid N^3 and precision (64, 32)
  n_gl, n_sph radial nodes (GaussLegendreQuadrature(n_gl, 0, 10)) and directions of a random rule without antipodal
              symmetry (bilinear_ref.random_rule(n_sph, seed=n)); n_gl * n_sph exceeds KA's direction groups at N
              (gain_spectra: groups_a), so KA's workgroups loop over two or more directions (all but the last
              one at N = 128, which gets one of 10)
  geometry    KA's form, in the words above
"""
from collections import namedtuple

Cube = namedtuple("Cube", "n prec n_gl n_sph geometry")

CUBES = [
    Cube(16, 64, 5, 14, "sequential, run-time sign, keep"),        # the plane-tile pipeline (the N = 16 whole-direction
    Cube(16, 32, 5, 14, "sequential, run-time sign, keep"),        # kernels have no bilinear form)
    Cube(24, 64, 4, 11, "pair, keep"),
    Cube(24, 32, 4, 11, "pair, keep"),
    Cube(32, 64, 5, 14, "32 x 64 panel, keep both planes"),
    Cube(32, 32, 5, 14, "32 x 64 panel, keep both planes"),
    Cube(40, 64, 2, 14, "pair, re-read"),                          # E = 20 points of 16 bytes: over the 256-byte cap
    Cube(40, 32, 2, 14, "pair, keep"),
    Cube(48, 64, 2, 12, "sequential, run-time sign, keep"),
    Cube(48, 32, 2, 12, "pair, keep"),
    Cube(64, 64, 2, 9, "pair, keep"),                              # cfg3
    Cube(64, 32, 2, 9, "sequential, compile-time sign, keep"),
    Cube(80, 64, 2, 5, "sequential, run-time sign, re-read"),
    Cube(80, 32, 2, 5, "sequential, run-time sign, re-read"),      # KEEP off for the bilinear form only
    Cube(96, 64, 2, 5, "pair, re-read"),
    Cube(96, 32, 2, 5, "pair, keep"),
    Cube(128, 64, 2, 5, "sequential, run-time sign, re-read, split"),   # the spilling instantiation
    Cube(128, 32, 2, 5, "pair, keep, pairs-il"),                   # cfg5
]

# Launch-sequence variants, at the cfg3 and cfg5 geometries and at N = 80 in single precision, each on the inputs of the
# cube case of its (N, precision):
#   chunks  max_chunk = 2, so that chunks cross radial-node boundaries (directions 8..9 at N = 64, 4..5 at N = 80 and
#           128), with more than 8 slabs: the separate Reduce launch.
#   single  one chunk with at most 8 slabs: the reduce fused into the tail (Pipeline::fuse_reduce).
# `chunks` is the n_chunks bfsm_get_counters reports (and so KA's launches), `slabs` the segments of the plan, `reduce` the
# kernel_launches[BFSM_K_REDUCE] of a profiled call.
Variant = namedtuple("Variant", "n prec max_chunk chunks slabs reduce")

VARIANTS = [
    Variant(64, 64, 2, 9, 18, 1), Variant(64, 64, 0, 1, 8, 0),
    Variant(128, 32, 2, 5, 10, 1), Variant(128, 32, 0, 1, 4, 0),
    Variant(80, 32, 2, 5, 10, 1), Variant(80, 32, 0, 1, 8, 0),
]
VARIANT_SIZES = ((64, 64), (128, 32), (80, 32))
# a handle created for batches (bfsm_desc.max_batch) running a single bilinear call.  At N >= 64 the per-distribution
# workgroup target stays at its floor of 512 (target_workgroups), so such a handle differs in its buffer sizes only; at
# N = 40 it also halves KA's direction groups and the segments, so the batch handle runs there as well.
BATCH_SIZES = VARIANT_SIZES + ((40, 64), (40, 32))
MAX_BATCH = 3


def cube(n, prec):
    (c,) = [c for c in CUBES if (c.n, c.prec) == (n, prec)]
    return c


def shards(n_dirs):
    """Three direction shards of uneven length covering [0, n_dirs); the GPU test adds the loss term on rank 0 only."""
    a, b = n_dirs // 5, n_dirs // 5 + n_dirs // 2
    return ((0, a), (a, b), (b, n_dirs))


def fused_sizes_of_pipeline(text):
    """The cube sizes of fused_grid() in the text of csrc/bfsm_pipeline.hpp."""
    import re
    body = re.search(r"inline bool fused_grid\(const bfsm_desc& d\) \{(.*?)\n\}", text, re.S).group(1)
    return sorted({int(v) for v in re.findall(r"N == (\d+)", body)})
