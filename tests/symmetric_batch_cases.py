"""Case table of the batched two-operand forms (include/bfsm.h, bfsm_collide_symmetric_batch*, bfsm_collide_bilinear_batch_partial_async):
member i of Q is Qs(g_i, f_i) or Q(g_i, f_i), with g or f optionally ONE array that every member reads.

Plain data, importable without a GPU: the smallest shapes that reach each kernel form of the batched sequence
(Pipeline::collide_pairs, csrc/bfsm_pipeline.hpp).  tests/test_emu_symmetric_batch.py runs the N <= 32 cases and the box under the
host emulator and checks the table against make_plan; tests/test_gpu_symmetric_batch.py runs every entry on the GPU.  The
reference is tests/symmetric_ref.py / tests/bilinear_ref.py per member on the full rule.

Modes as in tests/symmetric_cases.py.  The rule of a case is symmetric_ref.antipodal_rule(n_sph / 2, seed): merged to n_sph / 2
effective directions of doubled weight on the exact modes.  share: None, "g" or "f".

  N = 16, 24   three modes x two precisions, 2 radial nodes x a 2 x 3-point antipodal rule, max_batch 3 with n_batch 3, 2 and 1;
               the share values rotate so that every (N, precision, mode) sees all three.  KA = GainInv (GainInvBiBatchParams),
               on Hermitian handles with KN (NyqRowsBiBatchParams) as a launch of its own
  N = 32       fp64, Hermitian: the pair KA (body_gain_inv_pair) with a KN launch of its own
  N = 64       fp64, Hermitian, n_batch 2: GainInvNyq (GainInvNyqBiBatchParams) with guest KN rows in a batched grid; 5 x 7
               effective directions against the handle's KA groups (groups() below, the library's formula), so that KA's
               workgroups loop over two directions; fp64, faithful, n_batch 2
  N = 128      fp32, Hermitian, n_batch 2, share "f", 1 radial node x 4 points: GainInvTwo
  (12, 8, 20)  size-generic box, n_batch 2: member by member through the single calls
  variants     max_chunk = 2 crossing radial nodes with 2 x slabs > 8 (the separate reduce); a shard with 2 x slabs <= 8 (the
               reduce fused into the tail); both with n_batch 2
chunks / slabs: what make_plan must decide (fused cubes; slabs: the plan's segments, the symmetric call writes 2 x slabs per
member); reduce: kernel_launches[BFSM_K_REDUCE] of the symmetric call.
"""
from collections import namedtuple

EXACT, HERMITIAN = 2, 4                              # include/bfsm.h
MODES = {"faithful": 0, "exact": EXACT, "hermitian": EXACT | HERMITIAN}
SHARES = (None, "g", "f")
FUSE_LIMIT = 8                                       # Pipeline::fuse_reduce_symmetric: 2 * slab_count <= 8
MAX_BATCH = 3

Case = namedtuple("Case", "shape prec mode n_gl n_sph max_batch n_batch share max_chunk shard chunks slabs reduce")


def _small():
    out, k = [], 0
    for n in (16, 24):
        for mode in ("faithful", "exact", "hermitian"):
            for prec in (64, 32):
                slabs = 12 if mode == "faithful" else 6         # one segment per (effective) direction
                for j, nb in enumerate((3, 2, 1)):
                    out.append(Case(n, prec, mode, 2, 6, MAX_BATCH, nb, SHARES[(k + j) % 3], 0, None, 1, slabs, 1))
                k += 1
    return out


CASES = _small() + [
    Case(32, 64, "hermitian", 2, 6, 2, 2, "g", 0, None, 1, 6, 1),
    Case(64, 64, "hermitian", 5, 14, 2, 2, None, 0, None, 1, 35, 1),
    Case(64, 64, "faithful", 2, 6, 2, 2, "g", 0, None, 1, 8, 1),
    Case(128, 32, "hermitian", 1, 8, 2, 2, "f", 0, None, 1, 4, 0),
    Case((12, 8, 20), 64, "faithful", 2, 6, 2, 2, "f", 0, None, 0, 0, 0),
    # launch-sequence variants (N = 24, fp64, Hermitian, n_batch 2): chunks of 2 across 3 radial nodes; a shard of 3 effective
    # directions whose 2 x 3 slabs the tail reduces itself
    Case(24, 64, "hermitian", 3, 6, 2, 2, "f", 2, None, 5, 9, 1),
    Case(24, 64, "hermitian", 2, 6, 2, 2, "g", 0, (0, 6), 1, 3, 0),
]

EMU_CASES = [c for c in CASES if not isinstance(c.shape, int) or c.shape <= 32]


def groups(n, mode, max_batch):
    """KA's direction groups (Pipeline::gain_spectra, groups_a; target_workgroups with the handle's max_batch)."""
    single = 512 if n >= 64 else (2048 if n == 32 else 1024)
    target = max(single // max(max_batch, 1), 512)
    planes = n // 2 + 1 if mode == "hermitian" else n
    return max(target // planes, 1) * (2 if n == 64 else 1)


def sph_eff(c):
    return c.n_sph if c.mode == "faithful" or not isinstance(c.shape, int) else c.n_sph // 2


def cid(c):
    s = f"N{c.shape}" if isinstance(c.shape, int) else "x".join(str(v) for v in c.shape)
    extra = (f"-chunk{c.max_chunk}" if c.max_chunk else "") + (f"-shard{c.shard[0]}_{c.shard[1]}" if c.shard else "")
    return f"{s}-fp{c.prec}-{c.mode}-nb{c.n_batch}-share_{c.share or 'none'}{extra}"
