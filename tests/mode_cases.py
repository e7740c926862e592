"""Case table of the two reduction modes, BFSM_FLAG_EXACT_REDUCTIONS ("exact") and BFSM_FLAG_HERMITIAN on top of it
("hermitian"), on the fused cubes (csrc/bfsm_pipeline.hpp, fused_grid): every (N, precision, mode) with the kernel form it
compiles to and the launch-sequence variants the GPU suite runs on it, each with the plan it must take.

Plain data, importable without a GPU.  tests/test_emu_modes.py checks the table on the CPU (complete for fused_grid(), every
variant takes the plan it declares under the library's own make_plan) and runs the small sizes under the emulator;
tests/test_gpu_modes.py runs every entry on the GPU against the oracle.

Kernel forms, in the words of csrc/bfsm_core.hpp:
  KB'   body_gain_line_acc: the x-line kernel of the exact mode (segment sum of the products in registers)
  KB'H  body_gain_line_acc_h: the same on the stored planes lx = 0 .. N/2, the x-lines rebuilt from the half and the Nyquist
        rows.  "two-line": both lines of a direction loaded together; "one-line": one line at a time (N >= 128, to stay inside
        128 VGPRs).  "two-row blocks": a workgroup takes two whole rows of columns (N = 32, line_npl = 64).  "lane offset
        re-derived": the offset of the final stores is recomputed from the thread id (N = 32, 64).  "padded rows": the rows
        of line-kernel lanes are padded to 64 with duplicate lanes (row_pad of line_npl: N = 40, 48, 80, 96)
  KN    body_nyq_rows, the Nyquist rows of a chunk: "KN own launch", or "KN riding in KA" as guest rows of KA's grid
        (body_gain_inv_nyq, nyq_rides_along: N = 64)
  GainInvTwo    KA storing two arrays on the geometry whose default is interleaved {A1', A2'} pairs (N = 128 in single
        precision, Hermitian mode); the exact mode keeps the "interleaved pairs" there
  small_*       the whole-direction kernels of N = 16 (single evaluations on a handle without max_batch); with
        BFSM_FLAG_NO_SMALL_PATH, and on batch handles, N = 16 takes the plane-tile pipeline like every other size

Rules and inputs:
  "design"  the shipped 12-point design (antipodal: sph_eff = 6, weight x 2) with N_GL = 3 radial nodes, B = 36 full and 18
            effective directions
  "odd"     bilinear_ref.random_rule(9, seed=N): no antipodal symmetry, odd n_sph, with NOANTI_N_GL = 2 radial nodes: nothing
            is merged, 18 directions in both modes
  the field perturbed_input(bkw(N), amp = AMP[N]); the second batch member is another perturbation (BATCH_MEMBER_1)

A variant (kind, on every (N, precision, mode)):
  many     max_chunk = 4: five chunks of effective directions (4, 4, 4, 4, 2), the second, [4, 8), crossing the radial
           node at 6 (the fourth starts on the one at 12), more than 8 slabs: the separate Reduce launch
  few      the full-direction shard (12, 24) = the middle radial node (rho = 1.5, whose gain is of the order of max|Q|; the
           inner node's is 4 % of it), max_chunk = 4: two chunks of 3, six slabs: the reduce fused into TailInv
           (Pipeline::fuse_reduce); reference: the oracle's gain over the same directions, loss included
  shards   three uneven shards in full directions (0, 1), (1, 17), (17, 36), max_chunk = 3, loss on rank 0, summed after
           collidePartial.  (0, 1) maps to the empty effective range (0, 0); 17 lies inside the second radial node and
           17 * 6 % 12 != 0: the cut falls inside an antipodal pair's half and is floored to 8
  batch    a handle with max_batch = 3 running n_batch = 2, max_chunk = 5: chunks of 5, 5, 5, 3 (the last one shorter, so
           the batch strides of the scratch are those of the largest chunk, not of the chunk at hand)
  noanti   the "odd" rule, max_chunk = 5: chunks of 5, 5, 5, 3, the second crossing the radial node at 9
Each variant's parts (one per handle) declare n_chunks, chunk_dirs (the largest chunk), n_dirs, slabs and the reduce route
(kernel_launches[BFSM_K_REDUCE] of a profiled call: 1 above fuse_reduce()'s 8 slabs, else 0); SLABS holds the slab counts,
which depend on N and the precision (make_plan: segments per radial run).
"""
import math
from collections import namedtuple

EXACT, HERMITIAN, NO_SMALL_PATH = 2, 4, 8          # include/bfsm.h
MODES = {"exact": EXACT, "hermitian": EXACT | HERMITIAN}
PRECISIONS = (64, 32)
KINDS = ("many", "few", "shards", "batch", "noanti")

N_GL, N_SPH, SPH_EFF = 3, 12, 6
B = N_GL * N_SPH
NOANTI_N_GL, NOANTI_N_SPH = 2, 9
MAX_BATCH, N_BATCH = 3, 2
BATCH_MEMBER_1 = dict(seed=0xB2, amp=0.2)
FUSE_LIMIT = 8                                      # Pipeline::fuse_reduce: slab_count <= 8

# amplitude of perturbed_input per size: the default 0.1 unless the Nyquist planes of the input would not show at 100 x
# the fp32 bound in the reference alone (tests/test_emu_modes.py, test_each_case_can_fail_for_the_right_reason)
AMP = {16: 0.1, 24: 0.1, 32: 0.1, 40: 0.1, 48: 0.1, 64: 0.1, 80: 0.1, 96: 0.1, 128: 0.1}

_KBH = {16: "two-line KB'H", 24: "two-line KB'H", 32: "two-line KB'H, two-row blocks, lane offset re-derived",
        40: "two-line KB'H, padded rows", 48: "two-line KB'H, padded rows", 64: "two-line KB'H, lane offset re-derived",
        80: "two-line KB'H, padded rows", 96: "two-line KB'H, padded rows", 128: "one-line KB'H"}
_KB = {16: "KB'", 24: "KB'", 32: "KB', two-row blocks", 40: "KB', padded rows", 48: "KB', padded rows", 64: "KB'",
       80: "KB', padded rows", 96: "KB', padded rows", 128: "KB'"}


def _forms(n, prec, mode):
    if mode == "exact":
        s = _KB[n] + (", interleaved pairs" if (n, prec) == (128, 32) else "")
    else:
        s = ("KN riding in KA" if n == 64 else "KN own launch") + ", " + _KBH[n] + (", GainInvTwo" if (n, prec) == (128, 32) else "")
    return ("small_* whole-direction kernels; with BFSM_FLAG_NO_SMALL_PATH: " if n == 16 else "") + s


Case = namedtuple("Case", "n prec mode forms")
SIZES = (16, 24, 32, 40, 48, 64, 80, 96, 128)
CASES = [Case(n, prec, mode, _forms(n, prec, mode)) for n in SIZES for prec in PRECISIONS for mode in MODES]

# slabs (segments of the plan) per (N, precision): many, few, shards (one per rank), batch, noanti
# (chunks this short give one segment per direction, except where 5 directions meet the 4 workgroup columns of N = 128)
SLABS = {(n, prec): dict(many=18, few=6, shards=(0, 8, 10), batch=18, noanti=18) for n in SIZES[:-1] for prec in PRECISIONS}
SLABS.update({(128, prec): dict(many=18, few=6, shards=(0, 8, 10), batch=14, noanti=14) for prec in PRECISIONS})

# one handle of a variant: its shard in full directions (None: the whole handle) and the plan it must take
Part = namedtuple("Part", "shard n_chunks chunk_dirs n_dirs slabs reduce")
# small: N = 16 only: True = the handle may take the whole-direction kernels, False = BFSM_FLAG_NO_SMALL_PATH; None elsewhere
Variant = namedtuple("Variant", "kind n prec mode rule n_gl n_sph max_chunk max_batch n_batch merged small parts")

SHARDS = ((0, 1), (1, 17), (17, B))
# (n_chunks, chunk_dirs, n_dirs) of every part, in effective directions: the same at every size
_PLANS = {"many": ((None, 5, 4, 18),), "few": (((12, 24), 2, 3, 6),),
          "shards": ((SHARDS[0], 0, 0, 0), (SHARDS[1], 3, 3, 8), (SHARDS[2], 4, 3, 10)),
          "batch": ((None, 4, 5, 18),), "noanti": ((None, 4, 5, 18),)}
_MAX_CHUNK = {"many": 4, "few": 4, "shards": 3, "batch": 5, "noanti": 5}


def _variant(kind, c, small):
    slabs = SLABS[(c.n, c.prec)][kind]
    slabs = slabs if isinstance(slabs, tuple) else (slabs,)
    parts = tuple(Part(sh, nc, cd, nd, s, 1 if s > FUSE_LIMIT else 0) for (sh, nc, cd, nd), s in zip(_PLANS[kind], slabs))
    odd = kind == "noanti"
    return Variant(kind, c.n, c.prec, c.mode, "odd" if odd else "design", NOANTI_N_GL if odd else N_GL,
                   NOANTI_N_SPH if odd else N_SPH, _MAX_CHUNK[kind], MAX_BATCH if kind == "batch" else 0,
                   N_BATCH if kind == "batch" else 1, 0 if odd else 1, small, parts)


def _variants():
    out = []
    for c in CASES:
        for kind in KINDS:
            if c.n != 16:
                out.append(_variant(kind, c, None))
            else:       # a batch handle never takes the whole-direction kernels: one row
                out.extend(_variant(kind, c, small) for small in ((False,) if kind == "batch" else (True, False)))
    return out


VARIANTS = _variants()


def flags(v):
    """The descriptor flags of a variant."""
    return MODES[v.mode] | (NO_SMALL_PATH if v.small is False else 0)


def small_path_runs(v, part):
    """The part's single evaluations run on the whole-direction kernels (Pipeline::init: N = 16, no batch, directions)."""
    return v.n == 16 and v.small is True and v.max_batch <= 1 and part.n_dirs > 0


def launches(v, part):
    """(gain_inv, reduce) launches of one profiled call of the part.  KN's own launch is booked under gain_inv
    (Pipeline::gain_spectra), so the Hermitian mode shows two per chunk wherever KN does not ride in KA's grid."""
    if small_path_runs(v, part):
        return 0, 1                                 # SmallGain is booked under gain_line, SmallReduce under reduce
    kn_own = v.mode == "hermitian" and v.n != 64
    return part.n_chunks * (2 if kn_own else 1), part.reduce


def vid(v):
    return f"N{v.n}-fp{v.prec}-{v.mode}-{v.kind}" + ("" if v.small is None else ("-small" if v.small else "-tiles"))


# ---- inputs and references, shared by the CPU and the GPU module (O: the oracle module, oracle/oracle.py) ---------------

# gamma, b_gamma and (with the BKW field) L are bfsm.reference_constants().  The radial rule is Gauss-Legendre on [0, R_MAX]
# with R_MAX = 3, not the reference driver's 10: there the outer of three nodes lies at rho = 8.9, eight standard deviations
# of the relative velocity of the BKW state, and its directions carry 1e-6 of Q or less (oracle alone, N = 16 .. 128), so no
# case could notice that the last chunk or shard was lost.  On [0, 3] the nodes are 0.34, 1.5 and 2.66 and every direction
# weighs several per cent of max|Q| (tests/test_emu_modes.py, test_each_case_can_fail_for_the_right_reason).
GAMMA, B_GAMMA, R_MAX = 0.0, 1.0 / (4.0 * math.pi), 3.0

_IN = {}


def rule(O, v):
    """(x, y, z, w) of the variant's rule."""
    if v.rule == "design":
        return O.spherical_design(v.n_sph)
    import bilinear_ref
    return bilinear_ref.random_rule(v.n_sph, seed=v.n)


def inputs(O, n):
    """The field of size n, the second batch member and the box half-width L, computed once; refs: the references."""
    if n not in _IN:
        f0, _, L, _ = O.bkw(n)
        _IN[n] = dict(L=L, f=O.perturbed_input(f0, amp=AMP[n]), f1=O.perturbed_input(f0, **BATCH_MEMBER_1), refs={})
    return _IN[n]


def reference(O, v, member=0):
    """The oracle's Q of a variant (of its batch member) on the full rule: no merge, no Hermitian shortcut.  The "few"
    variant: the gain of its shard's directions and the loss.  Cached per (N, rule, shard, member); never modified."""
    inp = inputs(O, v.n)
    rng = v.parts[0].shard if v.kind == "few" else None
    key = (v.rule, v.n_gl, rng, member)
    if key not in inp["refs"]:
        gl = O.gauss_legendre(v.n_gl, 0.0, R_MAX)
        ref = O.collide(inp["f1" if member else "f"], gl, rule(O, v), GAMMA, B_GAMMA, inp["L"], dir_range=rng)
        ref.setflags(write=False)
        inp["refs"][key] = ref
    return inp["refs"][key]
