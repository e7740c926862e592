"""Chunkings of the size-generic path's fused sequence (csrc/bfsm_generic.hpp, gain_chunk_fused) that the GPU suite runs on
purpose: boxes with different plane-accumulate group limits (512 workgroups per launch over nx planes), each with
max_chunk values whose chunk lists launch different numbers of groups from chunk to chunk.

Plain data, importable without a GPU.  tests/test_generic_chunks.py proves on the CPU, from the launch recorder of the
emulator library (tests/emu/bfsm_emu.cpp, bfsm_emu_gen_routes, the GPU's grouping), that every entry launches exactly the
groups it declares and has the properties it declares, and that every property is declared per box kind and precision;
tests/test_gpu_generic_chunks.py runs every entry on the GPU and asserts n_chunks and the gain_fwd launch count there.

An entry:
  name       short id
  shape      (nx, ny, nz)
  n_gl, n_sph
  dir_range  direction shard of the handle, (0, 0) = all n_gl * n_sph directions
  max_chunk  bfsm_desc::max_chunk (0 = the path's default of 256)
  precs      precisions it runs in
  groups     plane-accumulate groups of the chunks in order: one launch per chunk, grid.y = groups (x members of a batch);
             len(groups) is the n_chunks and the gain_fwd launch count bfsm_get_counters reports for one evaluation
  props      what the entry is there for, see PROPS
"""
from collections import namedtuple

ChunkCase = namedtuple("ChunkCase", "name shape n_gl n_sph dir_range max_chunk precs groups props")

MORE = "a later chunk launches more groups than the first"        # the slab must be sized for the later chunk
FEWER = "a later chunk launches fewer groups than the first"
ONE = "max_chunk = 1"
SINGLE_LAST = "last chunk of a single direction"
BASELINE = "max_chunk = 0"
PROPS = (MORE, FEWER, ONE, SINGLE_LAST, BASELINE)

ALL = (0, 0)
BOTH = (64, 32)

CASES = [
    # 32 planes: at most 16 groups.  6 x 6 rule
    ChunkCase("c32x8x8-chunk17-of33", (32, 8, 8), 6, 6, (0, 33), 17, BOTH, (9, 16), (MORE,)),
    ChunkCase("c32x8x8-chunk16", (32, 8, 8), 6, 6, ALL, 16, BOTH, (16, 16, 4), (FEWER,)),
    ChunkCase("c32x8x8-chunk7", (32, 8, 8), 6, 6, ALL, 7, BOTH, (7, 7, 7, 7, 7, 1), (FEWER, SINGLE_LAST)),
    ChunkCase("c32x8x8-chunk1", (32, 8, 8), 6, 6, ALL, 1, BOTH, (1,) * 36, (ONE,)),
    ChunkCase("c32x8x8-chunk0", (32, 8, 8), 6, 6, ALL, 0, BOTH, (12,), (BASELINE,)),
    # 16 planes: at most 32 groups.  6 x 12 rule
    ChunkCase("c16x8x6-chunk40", (16, 8, 6), 6, 12, ALL, 40, BOTH, (20, 32), (MORE,)),
    ChunkCase("c16x8x6-chunk32", (16, 8, 6), 6, 12, ALL, 32, BOTH, (32, 32, 8), (FEWER,)),
    ChunkCase("c16x8x6-chunk71", (16, 8, 6), 6, 12, ALL, 71, BOTH, (24, 1), (FEWER, SINGLE_LAST)),
    ChunkCase("c16x8x6-chunk1", (16, 8, 6), 6, 12, ALL, 1, BOTH, (1,) * 72, (ONE,)),
    ChunkCase("c16x8x6-chunk0", (16, 8, 6), 6, 12, ALL, 0, BOTH, (24,), (BASELINE,)),
    # 100 planes: at most 6 groups; the 8-line x-line kernel in fp64.  6 x 6 rule
    ChunkCase("c100x4x6-chunk25", (100, 4, 6), 6, 6, ALL, 25, BOTH, (5, 6), (MORE,)),
    ChunkCase("c100x4x6-chunk7", (100, 4, 6), 6, 6, ALL, 7, BOTH, (4, 4, 4, 4, 4, 1), (FEWER, SINGLE_LAST)),
    ChunkCase("c100x4x6-chunk1", (100, 4, 6), 6, 6, ALL, 1, BOTH, (1,) * 36, (ONE,)),
    ChunkCase("c100x4x6-chunk0", (100, 4, 6), 6, 6, ALL, 0, BOTH, (6,), (BASELINE,)),
]


def n_dirs(case):
    b0, b1 = case.dir_range
    return case.n_gl * case.n_sph if (b0, b1) == ALL else b1 - b0


def complement(case):
    """The directions a shard entry leaves out (None for an entry that owns all)."""
    b0, b1 = case.dir_range
    B = case.n_gl * case.n_sph
    if (b0, b1) in (ALL, (0, B)):
        return None
    assert b0 == 0
    return (b1, B)


def recorded_groups(launches, nb=1):
    """Groups of the plane-accumulate launches of one recorded call (tests/emu_lib.py gen_routes), in order."""
    out = []
    for l in launches:
        if l["kind"] == "PlaneAcc":
            assert l["grid"][1] % nb == 0
            out.append(l["grid"][1] // nb)
    return tuple(out)


def properties(case, groups, chunks, chunk):
    """The PROPS a recorded plan has: groups = recorded_groups, chunks = [(dir0, n)], chunk = directions resident at once."""
    out = set()
    if any(g > groups[0] for g in groups[1:]):
        out.add(MORE)
    if any(g < groups[0] for g in groups[1:]):
        out.add(FEWER)
    if case.max_chunk == 1 and chunk == 1 and len(chunks) == n_dirs(case) > 1:
        out.add(ONE)
    if len(chunks) > 1 and chunk > 1 and chunks[-1][1] == 1:
        out.add(SINGLE_LAST)
    if case.max_chunk == 0 and len(chunks) == 1:
        out.add(BASELINE)
    return out
