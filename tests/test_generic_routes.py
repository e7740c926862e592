"""CPU checks of the size-generic path's kernel selection (csrc/bfsm_generic.hpp: pass_lines, line3_lines, plane_ok,
fused_ok, line3_ok, gen_table_radix) and of the case table tests/generic_cases.py that the GPU suite runs.

The launch recorder of the emulator library (tests/emu/bfsm_emu.cpp, bfsm_emu_gen_routes) runs GenericPipeline's own host
code for an entry point and records every launch -- kernel kind, precision, params type, load-side mode, grid, LDS --
without executing anything, with the GPU's plane-accumulate grouping.

  * census: a sweep over boxes whose extents cover every radix class and both sides of every threshold, in both
    precisions and through every entry point, collects the forms (kind, precision, bilinear, mode) the code can reach;
  * coverage: the case table declares exactly that set (plus the edges of generic_cases.EDGES), each target in exactly
    one case -- a new route without a GPU case, or a case that is no longer needed, fails here;
  * per case: the recorder reports the forms the case declares and exactly its kernel_launches;
  * forms the code cannot reach, stated so that a change of a threshold shows up here.
"""
import itertools

import pytest

import emu_lib as E
import generic_cases as GC

OPS = ("collide", "batch", "partial", "bilinear", "fft_fwd", "fft_bwd")
# extents of the census: every radix class (2^k, 3, 5, 7, 11, 13) and both sides of every threshold (8-line passes
# above 147 points in fp64, the 8-line x-line kernel from 100 points in fp64 and from 198 in fp32, the plane caps)
EXTENTS = (4, 6, 14, 22, 26, 60, 96, 98, 100, 128, 144, 150, 154, 160, 196, 198, 200, 240, 250, 252, 256)
PARTNERS = (4, 14, 60)          # small, radix 7 (no plane kernel), a plane over both caps once paired with itself
FUSED_CUBES = (16, 24, 32, 40, 48, 64, 80, 96, 128)


def _boxes():
    out = set()
    for e in EXTENTS:
        for a, b in itertools.product(PARTNERS, PARTNERS):
            out |= {(e, a, b), (a, e, b), (a, b, e)}
    out.add((16, 40, 60))
    return sorted(b for b in out if not (b[0] == b[1] == b[2] and b[0] in FUSED_CUBES))


def _call(box, prec, op):
    B = 2
    if op == "batch":
        return E.gen_routes(box, 1, B, prec, op, nb=2, max_batch=2)
    if op == "partial":
        return E.gen_routes(box, 1, B, prec, op, dir_range=(1, 2))
    return E.gen_routes(box, 1, B, prec, op, nb=2 if op.startswith("fft") else 1)


_CENSUS = None


def census():
    """{form: first box that reaches it}, and the per-box (launches, info) of the collide entry point."""
    global _CENSUS
    if _CENSUS is None:
        forms, boxes = {}, {}
        for box in _boxes():
            for prec in (64, 32):
                for op in OPS:
                    launches, _, info = _call(box, prec, op)
                    for l in launches:
                        forms.setdefault(GC.form(l), box)
                    if op == "collide":
                        boxes[(box, prec)] = (launches, info)
        _CENSUS = forms, boxes
    return _CENSUS


def _declared():
    out = []
    for c in GC.CASES:
        out += [(t, c.name) for t in c.targets]
    return out


def test_census_reaches_every_kind_in_both_precisions():
    forms = census()[0]
    kinds = {(f[0], f[1]) for f in forms}
    for k in E.GK_NAMES:
        assert (k, 64) in kinds, k
        if k not in ("Fft8", "FftBig8", "PlanePair"):     # (see test_forms_the_selection_code_cannot_reach)
            assert (k, 32) in kinds, k


def test_case_table_covers_every_reachable_route():
    """Every form the census reaches and every edge of generic_cases.EDGES is declared by a case; nothing else is."""
    forms = census()[0]
    required = set(forms) | set(GC.EDGES)
    declared = {t for t, _ in _declared()}
    missing = sorted(required - declared, key=str)
    assert not missing, "routes without a GPU case in tests/generic_cases.py: " + "; ".join(
        f"{t} (e.g. box {forms[t]})" if t in forms else str(t) for t in missing)
    extra = sorted(declared - required, key=str)
    assert not extra, f"case targets the census does not reach: {extra}"


def test_every_target_is_declared_once_and_every_case_is_needed():
    """Each target belongs to exactly one case, and every case has one: removing any case leaves a route uncovered."""
    seen = {}
    for t, name in _declared():
        assert t not in seen, f"{t} declared by {seen[t]} and {name}"
        seen[t] = name
    for c in GC.CASES:
        assert c.targets, f"case {c.name} declares no target: it is not needed"
        assert set(c.launches) == set(c.precs), c.name
        assert c.ops and c.ops[0] == "collide", c.name


@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c.name)
def test_case_takes_its_declared_route(case):
    """The recorder reports every target the case declares and exactly the kernel_launches it declares (the values the
    GPU test asserts through bfsm_get_counters)."""
    got = GC.recorded_targets(case, E.gen_routes)
    missing = sorted(set(case.targets) - got, key=str)
    assert not missing, f"{case.name} does not reach {missing}"
    for prec in case.precs:
        assert GC.collide_launches(case, prec, E.gen_routes) == tuple(case.launches[prec]), (case.name, prec)


def test_forms_the_selection_code_cannot_reach():
    """Recorded facts of csrc/bfsm_generic.hpp (the branches stay; a change of a threshold shows up here):
      * no 8-line pass in single precision: two 16-line buffers of 256 points and the twiddles are
        70 KiB <= 80 KiB, so Fft8 and FftBig8
        occur in double precision only;
      * the x-line kernel's LDS stays <= 80 KiB for every length <= 256 (16 lines, or 8 lines above 98 points in fp64
        and above 196 in fp32), so fused_ok() == plane_ok() && the x radices are 2, 3, 5 -- and the `if (pl) plane(...)`
        branches inside the x-line sequence of gain_spectra never run: gen_moves is never 8;
      * GEN_BETA2 is never a mode of any launch, and the plane kernel takes the phase multiply only in fp32, the
        plane-pair kernel only in fp64 (gain_chunk_fused: PAIR = sizeof(T) == 8)."""
    forms, boxes = census()
    assert not [f for f in forms if f[0] in ("Fft8", "FftBig8") and f[1] == 32]
    assert not [f for f in forms if f[3] == "BETA2"]
    assert ("Plane", 64, False, "PHASE") not in forms and ("Plane", 64, True, "PHASE") not in forms
    assert ("PlanePair", 32, False, "PHASE") not in forms and ("PlanePair", 32, True, "PHASE") not in forms
    for (box, prec), (launches, info) in boxes.items():
        table_x = any(box[0] % r == 0 for r in (7, 11, 13))
        assert info["fused"] == (info["plane"] and not table_x), (box, prec, info)
        assert info["gen_moves"] in (6, 12, 14, 18), (box, prec, info)
        kinds = [l["kind"] for l in launches]
        if ("Line3" in kinds or "Line38" in kinds) and "PlaneAcc" not in kinds:     # the x-line sequence, not fused
            assert not info["plane"] and "Plane" not in kinds, (box, prec)
    for n in GC.fft_lengths():
        if any(n % r == 0 for r in (7, 11, 13)):
            continue
        for prec in (64, 32):
            launches = E.gen_routes((n, 4, 4), 1, 2, prec)[0]
            (line,) = [l for l in launches if l["kind"] in ("Line3", "Line38")]
            assert line["lds"] <= 80 * 1024, (n, prec, line)
            assert line["kind"] == ("Line38" if n >= (100 if prec == 64 else 198) else "Line3"), (n, prec)


def test_pass_width_thresholds():
    """8 lines per workgroup in the per-axis passes exactly where two 16-line buffers and the twiddles pass 80 KiB:
    n >= 148 in fp64, never in fp32."""
    for n in GC.fft_lengths():
        for prec in (64, 32):
            launches = E.gen_routes((4, 14, n), 1, 2, prec, "fft_fwd")[0]
            z = launches[0]                        # the z pass comes first in the forward transform
            assert z["lds"] == (2 * n * (z["kind"].endswith("8") and 9 or 17) + n) * (16 if prec == 64 else 8), (n, prec)
            assert z["kind"].endswith("8") == (prec == 64 and n >= 148), (n, prec, z)
            assert z["kind"].startswith("FftBig") == any(n % r == 0 for r in (7, 11, 13)), (n, prec, z)
