"""Case table of the size-generic path (csrc/bfsm_generic.hpp): one entry per box that the GPU suite runs on purpose.

Plain data, importable without a GPU.  tests/test_generic_routes.py checks the table on the CPU against the launch
recorder of the emulator library (tests/emu/bfsm_emu.cpp, bfsm_emu_gen_routes): every case reaches the targets it
declares and launches exactly the kernels it declares; the cases together cover every route the selection code can
take; and no case is redundant.  tests/test_gpu_generic_routes.py runs every case on the GPU and asserts the declared
kernel_launches there, which proves that the GPU took the route the case claims.

A case:
  name       short id
  shape      (nx, ny, nz)
  n_gl, n_sph, max_chunk
  precs      precisions it runs in (64, 32)
  ops        entry points it exercises: "collide" (Q(f,f) against the oracle), "bilinear" (Q(g,f) against
             tests/bilinear_ref.py), "shards" (two direction shards, the loss term on rank 0), "batch" (a batch of two
             members against the single evaluations)
  targets    what the case is there to hit, each target declared by exactly one case:
               a form (kind, precision, bilinear, mode): the GK kernel kind, its precision, whether its params type is the
               bilinear one (GenFftBiParams), and its load-side mode (None for the kinds without one);
               an edge ("edge", name, precision or None), see EDGES
  launches   {precision: the six kernel_launches bfsm_get_counters reports for one bfsm_collide under BFSM_FLAG_PROFILE}
"""
from collections import namedtuple

Case = namedtuple("Case", "name shape n_gl n_sph max_chunk precs ops targets launches")

T, F = True, False

# edges: properties of a box that the form keys do not show
EDGE_Z256 = "plane kernels on a 256-point z line"          # dy = GEN_THREADS / nz = 1, dz = 0
EDGE_Y256 = "plane kernels on a 256-point y line"          # in double precision exactly at the 40 KiB plane cap
EDGE_PREC = "route depends on the precision"               # plane cap 1280 points in fp64, 2560 in fp32
EDGE_CROSS = "plane-accumulate groups straddle radial nodes under the GPU grouping"
EDGES = (("edge", EDGE_Z256, 64), ("edge", EDGE_Z256, 32), ("edge", EDGE_Y256, 64), ("edge", EDGE_Y256, 32),
         ("edge", EDGE_PREC, None), ("edge", EDGE_CROSS, 64), ("edge", EDGE_CROSS, 32))

CASES = [
    # fp64: per-axis passes around the x-line kernel (a 2400-point plane is over the 1280-point cap); fp32: the fused sequence
    Case("c16x40x60", (16, 40, 60), 2, 6, 0, (64, 32), ("collide", "bilinear"),
         (("Acc", 32, F, None), ("Acc", 64, F, None), ("Combine", 32, F, None), ("Combine", 64, F, None),
          ("Fft", 32, F, "PLAIN"), ("Fft", 32, F, "TAIL2"), ("Fft", 64, F, "PHASE"), ("Fft", 64, F, "PLAIN"),
          ("Fft", 64, F, "REAL"), ("Fft", 64, F, "TAIL2"), ("Fft", 64, T, "PHASE"), ("Line3", 32, F, None),
          ("Line3", 64, F, None), ("Plane", 32, F, "PHASE"), ("Plane", 32, F, "PLAIN"), ("Plane", 32, F, "REAL"),
          ("Plane", 32, T, "PHASE"), ("PlaneAcc", 32, F, None), ("edge", EDGE_PREC, None)),
         {64: (3, 2, 3, 1, 0, 4), 32: (2, 1, 1, 1, 1, 3)}),
    # fused sequence with 256-point z lines in the plane kernels (plane-accumulate: 49 KiB of LDS in fp64)
    Case("c8x4x256", (8, 4, 256), 2, 6, 0, (64, 32), ("collide", "bilinear", "shards", "batch"),
         (("Plane", 64, F, "PLAIN"), ("Plane", 64, F, "REAL"), ("PlaneAcc", 64, F, None), ("PlanePair", 64, F, "PHASE"),
          ("PlanePair", 64, T, "PHASE"), ("edge", EDGE_Z256, 32), ("edge", EDGE_Z256, 64)),
         {64: (2, 1, 1, 1, 1, 3), 32: (2, 1, 1, 1, 1, 3)}),
    # ... with 256-point y lines: 2 x 256 x 5 x 16 B = 40 KiB, exactly the plane cap in fp64
    Case("c8x256x4", (8, 256, 4), 2, 6, 0, (64, 32), ("collide", "bilinear"),
         (("edge", EDGE_Y256, 32), ("edge", EDGE_Y256, 64)),
         {64: (2, 1, 1, 1, 1, 3), 32: (2, 1, 1, 1, 1, 3)}),
    # 8-line x-line kernel in fp64 (three 16-line buffers: 83 200 B > 80 KiB); 30 directions in 6 groups of 5 across
    # radial nodes of 6 directions
    Case("c100x4x6", (100, 4, 6), 5, 6, 0, (64,), ("collide", "shards", "batch"),
         (("Line38", 64, F, None), ("edge", EDGE_CROSS, 64)),
         {64: (2, 1, 1, 1, 1, 3)}),
    # fp64: 8-line x passes (Q(f,f) through Fft8); fp32: the 8-line x-line kernel (nx >= 198), 3 groups of 4 directions
    Case("c200x4x4", (200, 4, 4), 2, 6, 0, (64, 32), ("collide", "bilinear", "shards", "batch"),
         (("Fft8", 64, F, "PLAIN"), ("Fft8", 64, F, "TAIL2"), ("Line38", 32, F, None), ("edge", EDGE_CROSS, 32)),
         {64: (2, 1, 1, 1, 1, 3), 32: (2, 1, 1, 1, 1, 3)}),
    # 154 = 2 x 7 x 11 on x: the table-driven radices on the 8-line x passes in fp64, on 16 lines in fp32
    Case("c154x4x4", (154, 4, 4), 2, 6, 0, (64, 32), ("collide", "bilinear", "shards", "batch"),
         (("FftBig", 32, F, "PHASE"), ("FftBig", 32, F, "PLAIN"), ("FftBig", 32, F, "TAIL2"), ("FftBig", 32, T, "PHASE"),
          ("FftBig8", 64, F, "PHASE"), ("FftBig8", 64, F, "PLAIN"), ("FftBig8", 64, F, "TAIL2"),
          ("FftBig8", 64, T, "PHASE"), ("Plane", 32, F, "PRODUCT"), ("Plane", 64, F, "PRODUCT")),
         {64: (2, 2, 2, 1, 0, 3), 32: (2, 2, 2, 1, 0, 3)}),
    # radix-7 y axis (no plane kernel), 160-point z passes: 8 lines in fp64, 16 in fp32
    Case("c4x14x160", (4, 14, 160), 2, 6, 0, (64, 32), ("collide", "bilinear", "shards", "batch"),
         (("Fft", 32, F, "PHASE"), ("Fft", 32, F, "REAL"), ("Fft", 32, T, "PHASE"), ("Fft8", 64, F, "PHASE"),
          ("Fft8", 64, F, "REAL"), ("Fft8", 64, T, "PHASE"), ("FftBig", 64, F, "PLAIN")),
         {64: (3, 2, 3, 1, 0, 4), 32: (3, 2, 3, 1, 0, 4)}),
    # radix-7 x axis (one pass per axis), the product formed on the load side of an 8-line z pass
    Case("c14x14x160", (14, 14, 160), 2, 6, 0, (64,), ("collide",),
         (("Fft8", 64, F, "PRODUCT"), ("FftBig", 64, F, "PHASE"), ("FftBig", 64, F, "TAIL2")),
         {64: (3, 3, 3, 1, 0, 4)}),
    # ... and of an 8-line z pass with the table-driven radices (154 = 2 x 7 x 11)
    Case("c14x4x154", (14, 4, 154), 2, 6, 0, (64,), ("collide", "bilinear"),
         (("FftBig", 64, T, "PHASE"), ("FftBig8", 64, F, "PRODUCT"), ("FftBig8", 64, F, "REAL")),
         {64: (3, 3, 3, 1, 0, 4)}),
    # radices 7, 11, 13 on the three axes
    Case("c14x22x26", (14, 22, 26), 2, 6, 0, (64, 32), ("collide", "bilinear"),
         (("FftBig", 32, F, "PRODUCT"), ("FftBig", 32, F, "REAL"), ("FftBig", 64, F, "PRODUCT"), ("FftBig", 64, F, "REAL")),
         {64: (3, 3, 3, 1, 0, 4), 32: (3, 3, 3, 1, 0, 4)}),
    # radix-11 x axis, radix-7 y axis: the product on the load side of a z pass without the table-driven radices
    Case("c22x14x6", (22, 14, 6), 2, 6, 0, (64, 32), ("collide",),
         (("Fft", 32, F, "PRODUCT"), ("Fft", 64, F, "PRODUCT")),
         {64: (3, 3, 3, 1, 0, 4), 32: (3, 3, 3, 1, 0, 4)}),
]


def shard_ranges(case):
    """The two direction shards of the "shards" entry point: halves of the case's directions."""
    B = case.n_gl * case.n_sph
    return (0, B // 2), (B // 2, B)


def _calls(case, prec):
    """(op, keyword arguments) of the recorder calls that stand for the case's entry points."""
    kw = dict(max_chunk=case.max_chunk)
    for op in case.ops:
        if op == "collide":
            yield "collide", dict(kw)
        elif op == "bilinear":
            yield "bilinear", dict(kw)
        elif op == "shards":
            r0, r1 = shard_ranges(case)
            yield "collide", dict(kw, dir_range=r0)
            yield "partial", dict(kw, dir_range=r1)
        elif op == "batch":
            yield "batch", dict(kw, nb=2, max_batch=2)
        else:
            raise ValueError(op)


def form(launch):
    return (launch["kind"], launch["precision"], launch["bilinear"], launch["mode"])


def crosses_radial_nodes(case, launches):
    """A plane-accumulate launch of the first chunk whose groups of consecutive directions span two radial nodes."""
    B = case.n_gl * case.n_sph
    n = min(case.max_chunk or 256, B)
    for l in launches:
        if l["kind"] != "PlaneAcc":
            continue
        groups = l["grid"][1]
        per = -(-n // groups)
        for g in range(groups):
            d0, d1 = g * per, min(n, (g + 1) * per)
            if d0 < d1 and d0 // case.n_sph != (d1 - 1) // case.n_sph:
                return True
    return False


def recorded_targets(case, routes):
    """Every target the case's entry points reach, from routes = tests/emu_lib.py gen_routes."""
    out = set()
    kinds = {}
    plane_kinds = {"Plane", "PlanePair", "PlaneAcc"}
    for prec in case.precs:
        for op, kw in _calls(case, prec):
            launches = routes(case.shape, case.n_gl, case.n_sph, prec, op, **kw)[0]
            out |= {form(l) for l in launches}
            if any(l["kind"] in plane_kinds for l in launches):
                if case.shape[2] == 256:
                    out.add(("edge", EDGE_Z256, prec))
                if case.shape[1] == 256:
                    out.add(("edge", EDGE_Y256, prec))
            if op == "collide" and "dir_range" not in kw:
                kinds[prec] = {l["kind"] for l in launches}
                if crosses_radial_nodes(case, launches):
                    out.add(("edge", EDGE_CROSS, prec))
    if len(kinds) == 2 and kinds[64] != kinds[32]:
        out.add(("edge", EDGE_PREC, None))
    return out


def collide_launches(case, prec, routes):
    """kernel_launches of one bfsm_collide of the case, from the recorder."""
    return routes(case.shape, case.n_gl, case.n_sph, prec, "collide", max_chunk=case.max_chunk)[1]


def fft_lengths():
    """Every axis length the size-generic path serves (csrc/bfsm_generic.hpp gen_factor / gen_supported): even, 4 to 256,
    prime factors up to 13, at most 8 radix passes (8, 4, 2 for the power of two, then 3, 5, 7, 11, 13 one by one)."""
    out = []
    for n in range(4, 257, 2):
        m, k2 = n, 0
        while m % 2 == 0:
            m //= 2
            k2 += 1
        passes = (k2 + 2) // 3
        for r in (3, 5, 7, 11, 13):
            while m % r == 0:
                m //= r
                passes += 1
        if m == 1 and passes <= 8:
            out.append(n)
    return out


def fft_boxes(n):
    """Where the FFT sweep puts an axis of length n: the x pass, the plane (y and z), and the per-axis y / z passes (a
    radix-7 partner axis keeps the plane kernel out)."""
    return [(n, 4, 4), (4, n, 4), (4, 4, n), (4, n, 14), (4, 14, n)]
