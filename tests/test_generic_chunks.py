"""CPU checks of how the size-generic path's fused sequence (csrc/bfsm_generic.hpp, GenericPipeline::init and
gain_chunk_fused) cuts a shard into chunks of directions, against what init allocated for them.

bfsm_desc::max_chunk "bounds scratch, not results".  The fused sequence owns two chunk-sized buffers: the A1 / A2 scratch
([mb][2 chunk][G]) and the plane-accumulate slab buffer ([mb][slab_groups][G]); every chunk is launched with
groups_for(chunk length) groups, and groups_for is not monotone: a shorter last chunk can ask for more groups than a full
one (32 planes, 17 directions: 9 groups of 2; 16 directions: 16 groups of 1).

The launch recorder of the emulator library (tests/emu/bfsm_emu.cpp, bfsm_emu_gen_routes) runs GenericPipeline's own host
code -- init included -- records every launch and what init allocated, allocates no scratch and executes nothing.

  * plan against allocation: a sweep over fused boxes (nx, 4, 4), every even nx <= 256 without the table-driven radices,
    both precisions, the entry points collide / partial / batch / bilinear, max_chunk 1..260, last chunks of every length,
    batches that make the 32767 / mb clamp act, under both groupings (512 workgroups per launch as on the GPU, 24 as in
    the emulator's numeric tests).  From the records alone: no plane-accumulate launch writes past the slab buffer, the
    accumulate launch after it sums exactly the slabs written, the chunks tile the shard, none is longer than the scratch
    holds, no grid dimension exceeds 65535.
  * the case table tests/generic_chunk_cases.py that the GPU suite runs: every entry launches the groups and has the
    properties it declares; every property is declared for every box and precision.

How the sweep is thinned (nothing executes, but init builds its phase tables, about a microsecond per direction and point):
SWEEP_NX of the x extents get every max_chunk 1..260 with last chunks of 1 direction, of one direction less than a full
chunk, none (the chunks divide the shard), and the two picked as below; the other extents get THIN_CHUNKS in the same way.
On top of that EVERY extent gets every max_chunk for which arithmetic on groups_for (groups_mirror below, itself checked
against every recorded launch) predicts that some shorter last chunk needs more groups than a full one, with the shortest
such last chunk through all four entry points (the precision alternates from pair to pair) and with the one that needs the
most groups.  The other plans take precision, entry point and batch size in turn.  REMAINDER_NX get every last chunk
length 1..259.
"""
import functools
import itertools

import pytest

import emu_lib as E
import generic_cases as GC
import generic_chunk_cases as CC

NXS = [n for n in GC.fft_lengths() if all(n % r for r in (7, 11, 13))]      # x radices 2, 3, 5: fused_ok() where the plane fits
SWEEP_NX = (4, 16, 32)
REMAINDER_NX = (16, 100)
THIN_CHUNKS = (1, 2, 3, 4, 5, 7, 8, 16, 17, 31, 32, 33, 64, 100, 127, 128, 129, 163, 164, 200, 255, 256, 257, 260)
CHUNKS = range(1, 261)
WGS = {True: 512, False: 24}          # gpu_groups -> BFSM_GEN_TARGET_WGS of the emulator build
# (entry point, members of the call, max_batch of the handle); 200 members: 32767 / mb = 163 directions at most
CALLS = (("collide", 1, 0), ("partial", 1, 0), ("bilinear", 1, 0), ("batch", 2, 2), ("batch", 3, 3), ("collide", 1, 2),
         ("batch", 2, 200), ("batch", 200, 200), ("partial", 1, 3), ("bilinear", 1, 128))
FOUR_OPS = (("collide", 1, 0), ("partial", 1, 0), ("bilinear", 1, 0), ("batch", 2, 2))
N_GL, N_SPH = 1, 540                  # shards (0, nd) of 540 directions leave any last chunk wanted


def groups_mirror(nx, n, wgs):
    """groups_for of csrc/bfsm_generic.hpp, restated: used to choose what the sweep records, and checked against every
    recorded launch."""
    g = max(1, min((wgs + nx - 1) // nx, n))
    per = (n + g - 1) // g
    return (n + per - 1) // per


@functools.lru_cache(maxsize=None)
def ragged_remainders(nx, chunk, wgs):
    """Lengths of a last chunk that needs more groups than a chunk of `chunk` directions: (shortest, the one with the most
    groups), or () if there is none."""
    full = groups_mirror(nx, chunk, wgs)
    worse = [r for r in range(1, chunk) if groups_mirror(nx, r, wgs) > full]
    if not worse:
        return ()
    return (worse[0], max(worse, key=lambda r: (groups_mirror(nx, r, wgs), -r)))


def _plans(nx, wgs):
    """[(max_chunk, last chunk length or 0, through all four entry points?)] of one x extent."""
    out = []
    for c in CHUNKS:
        ragged = ragged_remainders(nx, c, wgs)
        for r in dict.fromkeys(ragged):
            out.append((c, r, r == ragged[0]))
        if nx in SWEEP_NX or c in THIN_CHUNKS:
            for r in dict.fromkeys((0, 1, c - 1)):
                if 0 <= r < c and r not in ragged:
                    out.append((c, r, False))
    if nx in REMAINDER_NX:
        out += [(r + 1, r, False) for r in range(1, 260) if (r + 1, r, False) not in out]
    return out


def check_plan(launches, info, nb, nd, max_chunk, max_batch):
    """(hard errors, slab violations) of one recorded call, from the records alone."""
    errs, over = [], []
    chunks = info["chunks"]
    if not info["fused"]:
        return ["not on the fused sequence"], over
    mb = info["mb"]
    if mb != (max_batch if max_batch > 1 else 1):
        errs.append(f"scratch for {mb} members on a max_batch = {max_batch} handle")
    if info["slab_arrays"] != info["slab_groups"] * mb:
        errs.append(f"slab allocation of {info['slab_arrays']} arrays, slab_groups {info['slab_groups']} x {mb} members")
    if not 1 <= info["chunk"] <= min(max_chunk or 256, 32767 // mb):
        errs.append(f"chunk {info['chunk']} with max_chunk {max_chunk}, {mb} members")
    pos = 0
    for d0, n in chunks:                                  # the chunks tile the shard, each within the A1 / A2 scratch
        if d0 != pos or not 1 <= n <= info["chunk"]:
            errs.append(f"chunk ({d0}, {n}) at direction {pos}, scratch for {info['chunk']} directions")
        pos += n
    if pos != nd:
        errs.append(f"chunks cover {pos} of {nd} directions")
    for l in launches:
        if max(l["grid"]) > 65535 or min(l["grid"]) < 1:
            errs.append(f"{l['kind']} grid {l['grid']}")
    acc_at = [i for i, l in enumerate(launches) if l["kind"] == "PlaneAcc"]
    if len(acc_at) != len(chunks):
        errs.append(f"{len(acc_at)} plane-accumulate launches for {len(chunks)} chunks")
    for i, (d0, n) in zip(acc_at, chunks):
        l, nxt = launches[i], launches[i + 1]
        if (l["dir0"], l["n"]) != (d0, n):
            errs.append(f"plane-accumulate of directions ({l['dir0']}, {l['n']}) for chunk ({d0}, {n})")
        if l["grid"][1] != l["groups"] * nb or l["mgroups"] != l["groups"]:
            errs.append(f"plane-accumulate grid {l['grid']}: {l['groups']} groups, member distance {l['mgroups']}, {nb} members")
        if l["grid"][1] > info["slab_groups"] * nb:
            over.append(f"chunk ({d0}, {n}): grid.y {l['grid'][1]} > slab_groups {info['slab_groups']} x {nb}")
        if (nxt["kind"], nxt["groups"], nxt["mgroups"], nxt["grid"][1]) != ("Acc", l["groups"], l["mgroups"], nb):
            errs.append(f"after {l['groups']} groups (member distance {l['mgroups']}, {nb} members): {nxt}")
    return errs, over


def _record(nx, prec, call, max_chunk, nd, gpu_groups):
    op, nb, max_batch = call
    launches, _, info = E.gen_routes((nx, 4, 4), N_GL, N_SPH, prec, op, nb=nb, max_chunk=max_chunk, dir_range=(0, nd),
                                     max_batch=max_batch, gpu_groups=gpu_groups)
    return launches, info


@pytest.mark.parametrize("gpu_groups", [True, False], ids=["grouping512", "grouping24"])
def test_no_chunk_outgrows_what_init_allocated(gpu_groups):
    wgs = WGS[gpu_groups]
    turn = itertools.cycle(itertools.product((64, 32), CALLS))
    plans = bad_plans = predicted = 0
    first_bad, hard = [], []
    for nx in NXS:
        for max_chunk, r, four in _plans(nx, wgs):
            nd = max_chunk + r if r else 2 * max_chunk
            predicted += four
            for prec, call in ([((64, 32)[predicted % 2], c) for c in FOUR_OPS] if four else (next(turn),)):
                launches, info = _record(nx, prec, call, max_chunk, nd, gpu_groups)
                errs, over = check_plan(launches, info, call[1], nd, max_chunk, call[2])
                for l in launches:                                   # the arithmetic that chose the plans is the code's
                    if l["kind"] == "PlaneAcc" and l["groups"] != groups_mirror(nx, l["n"], wgs):
                        errs.append(f"groups_for({l['n']}) = {l['groups']}, restated as {groups_mirror(nx, l['n'], wgs)}")
                plans += 1
                where = f"({nx}, 4, 4) fp{prec} {call} max_chunk {max_chunk}, {nd} directions"
                hard += [f"{where}: {e}" for e in errs]
                if over:
                    bad_plans += 1
                    if len(first_bad) < 5:
                        first_bad.append(f"{where}: {over[0]}")
    print(f"grouping {wgs}: {plans} plans recorded, {predicted} (nx, max_chunk) pairs with a ragged last chunk, "
          f"{bad_plans} plans write past the slab buffer")
    assert not hard, f"{len(hard)} plan errors, e.g. {hard[:5]}"
    assert not bad_plans, (f"{bad_plans} of {plans} recorded plans launch a plane-accumulate grid that the slab buffer does not "
                           f"hold ({predicted} (nx, max_chunk) pairs), e.g. {first_bad}")


def test_where_a_last_chunk_needs_more_groups():
    """Recorded facts of groups_for under the GPU's grouping (a change of the grouping shows up here): over every even nx
    4..256 and max_chunk 1..256, 3751 of the 32512 pairs have a shorter last chunk that needs more groups than a full one;
    none at the default of 256 -- which is why no default plan ever met an undersized slab buffer.  The sweep above
    records every such pair of its extents."""
    pairs = [(nx, c) for nx in range(4, 257, 2) for c in range(1, 257) if ragged_remainders(nx, c, 512)]
    assert len(pairs) == 3751
    assert not [nx for nx, c in pairs if c == 256]
    swept = {(nx, c) for nx in NXS for c, r, four in _plans(nx, 512) if four and r == ragged_remainders(nx, c, 512)[0]}
    assert swept == {(nx, c) for nx in NXS for c in CHUNKS if ragged_remainders(nx, c, 512)}
    assert len(swept) == 2272
    for nx in NXS:
        assert {r for c, r, _ in _plans(nx, 512)} >= ({0, 1} | (set(range(1, 260)) if nx in REMAINDER_NX else set()))


CASE_PRECS = [pytest.param(c, p, id=f"{c.name}-fp{p}") for c in CC.CASES for p in c.precs]


@pytest.mark.parametrize("case,prec", CASE_PRECS)
def test_gpu_chunk_case_is_what_it_declares(case, prec):
    """The recorder (GPU grouping) reports the groups the entry declares, chunk by chunk, the properties it declares and no
    other, and one gain_fwd launch per chunk; the entry points the GPU test runs on the entry take the same chunks."""
    kw = dict(max_chunk=case.max_chunk, dir_range=case.dir_range)
    nd = CC.n_dirs(case)
    launches, kl, info = E.gen_routes(case.shape, case.n_gl, case.n_sph, prec, "collide", **kw)
    errs, over = check_plan(launches, info, 1, nd, case.max_chunk, 0)
    assert not errs and not over, (errs, over)
    groups = CC.recorded_groups(launches)
    assert groups == tuple(case.groups)
    assert CC.properties(case, groups, info["chunks"], info["chunk"]) == set(case.props)
    assert len(info["chunks"]) == len(case.groups) == kl[3]                  # n_chunks and kernel_launches[BFSM_K_GAIN_FWD]
    if CC.MORE in case.props:
        assert max(groups) > groups_mirror(case.shape[0], info["chunk"], 512)    # more than a slab sized for a full chunk holds
        for op, nb, max_batch in (("partial", 1, 0), ("bilinear", 1, 0), ("batch", 2, 2), ("collide", 1, 2)):
            launches, _, info = E.gen_routes(case.shape, case.n_gl, case.n_sph, prec, op, nb=nb, max_batch=max_batch, **kw)
            errs, over = check_plan(launches, info, nb, nd, case.max_chunk, max_batch)
            assert not errs and not over, (op, errs, over)
            assert CC.recorded_groups(launches, nb) == tuple(case.groups), op
        rest = CC.complement(case)
        if rest:
            launches, _, info = E.gen_routes(case.shape, case.n_gl, case.n_sph, prec, "partial", max_chunk=case.max_chunk, dir_range=rest)
            errs, over = check_plan(launches, info, 1, rest[1] - rest[0], case.max_chunk, 0)
            assert not errs and not over, (errs, over)


def test_gpu_chunk_cases_declare_every_property_per_box_and_precision():
    """Otherwise the GPU cases could be in bounds by accident, as the chunked cases before them were."""
    boxes = {c.shape for c in CC.CASES}
    assert len({(512 + s[0] - 1) // s[0] for s in boxes}) == len(boxes) >= 3      # different group limits
    for shape in boxes:
        for prec in (64, 32):
            declared = set()
            for c in CC.CASES:
                if c.shape == shape and prec in c.precs:
                    declared |= set(c.props)
            assert declared == set(CC.PROPS), (shape, prec, sorted(set(CC.PROPS) - declared))
    assert any(c.shape[0] >= 100 and 64 in c.precs for c in CC.CASES)             # the 8-line x-line kernel in fp64
