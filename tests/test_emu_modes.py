"""CPU tests of the two reduction modes (BFSM_FLAG_EXACT_REDUCTIONS, BFSM_FLAG_HERMITIAN) behind the GPU table
tests/mode_cases.py.

The table is complete for fused_grid() and every variant takes the plan it declares under the library's own make_plan; the
plan's effective-direction bookkeeping (antipodal merge, proportional shard map, chunks, segments) is checked over a wide
domain of rules, shards and chunk sizes; the variants of N = 16 and 24 run under the host lock-step emulator (same bodies,
same plan and launch sequence as the GPU) against the oracle in both precisions; and the oracle alone shows that each GPU
case would notice a missing direction and a wrong treatment of the input's Nyquist planes.
"""
import os
import re

import numpy as np
import pytest

import bilinear_cases as BC
import bilinear_ref as BR
import emu_lib as E
import mode_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "boltzmann-fourier-spectral-method_amd")
GAMMA, B_GAMMA, R = MC.GAMMA, MC.B_GAMMA, MC.R_MAX
TOL64, TOL32 = 1e-12, 5e-6                               # the GPU suite's bounds (tests/test_gpu_parity.py)
EMU_SIZES = (16, 24)


def _text(name):
    return open(os.path.join(PKG, "csrc", name)).read()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- the table -----------------------------------------------------------------------------------------------------

def test_table_is_complete():
    """Every cube size of fused_grid() x precision x mode has a case with its kernel form and every variant kind; N = 16
    runs every single-evaluation kind on the whole-direction kernels and on the plane-tile pipeline."""
    sizes = BC.fused_sizes_of_pipeline(_text("bfsm_pipeline.hpp"))
    assert 16 in sizes and 128 in sizes, sizes
    required = {(n, p, m) for n in sizes for p in MC.PRECISIONS for m in MC.MODES}
    declared = [(c.n, c.prec, c.mode) for c in MC.CASES]
    assert len(declared) == len(set(declared))
    assert not required - set(declared), f"fused cubes without a reduction-mode case: {sorted(required - set(declared))}"
    assert not set(declared) - required, f"cases that are not fused cubes: {sorted(set(declared) - required)}"
    assert set(MC.AMP) == set(sizes)
    core = _text("bfsm_core.hpp")
    assert re.search(r"nyq_rides_along\(\) \{.*?return N == 64 &&", core, re.S)
    assert "constexpr bool ONE_LINE = N >= 128;" in core
    for c in MC.CASES:
        kinds = [(v.kind, v.small) for v in MC.VARIANTS if (v.n, v.prec, v.mode) == (c.n, c.prec, c.mode)]
        if c.n == 16:
            want = [(k, s) for k in MC.KINDS for s in ((False,) if k == "batch" else (True, False))]
            assert "small_*" in c.forms and "NO_SMALL_PATH" in c.forms
        else:
            want = [(k, None) for k in MC.KINDS]
        assert sorted(kinds, key=str) == sorted(want, key=str), c
        if c.mode == "hermitian":
            assert ("KN riding in KA" in c.forms) == (c.n == 64) and ("KN own launch" in c.forms) == (c.n != 64), c
            assert ("one-line KB'H" in c.forms) == (c.n >= 128) and ("two-line KB'H" in c.forms) == (c.n < 128), c
            assert ("GainInvTwo" in c.forms) == ((c.n, c.prec) == (128, 32)), c
        else:
            assert "KB'" in c.forms and "KN" not in c.forms and "KB'H" not in c.forms, c
        assert ("two-row blocks" in c.forms) == (c.n == 32) and ("padded rows" in c.forms) == (c.n in (40, 48, 80, 96)), c


def test_every_variant_takes_its_declared_plan(oracle):
    """Chunks, largest chunk, effective directions and slabs of every part under make_plan with the variant's flags and
    rule, and so the reduce route; and the properties each kind is in the table for."""
    limit = int(re.search(r"bool fuse_reduce\(\) const \{ return slab_count <= (\d+); \}", _text("bfsm_pipeline.hpp")).group(1))
    assert limit == MC.FUSE_LIMIT
    assert MC.VARIANTS
    for v in MC.VARIANTS:
        sph = MC.rule(oracle, v)
        sph_eff = v.n_sph // 2 if v.merged else v.n_sph
        for p in v.parts:
            chunks, segs = E.plan(v.n, v.n_gl, v.n_sph, v.prec, p.shard or (0, 0), v.max_chunk, flags=MC.flags(v), sph=sph,
                                  max_batch=v.max_batch)
            n_dirs = sum(c[2] for c in chunks)
            got = (len(chunks), max([c[2] for c in chunks], default=0), n_dirs, len(segs))
            assert got == (p.n_chunks, p.chunk_dirs, p.n_dirs, p.slabs), (MC.vid(v), p, got)
            assert p.reduce == (1 if p.slabs > limit else 0), (MC.vid(v), p)
            b0, b1 = p.shard or (0, v.n_gl * v.n_sph)
            e0 = b0 * sph_eff // v.n_sph
            assert n_dirs == b1 * sph_eff // v.n_sph - e0
            crossing = [c for c in chunks if (e0 + c[1]) // sph_eff != (e0 + c[1] + c[2] - 1) // sph_eff]
            if v.kind in ("many", "noanti"):
                assert crossing, MC.vid(v)
        p0 = v.parts[0]
        if v.kind == "many":
            assert p0.n_chunks >= 3 and p0.slabs > limit and v.merged == 1
        elif v.kind == "few":
            assert p0.slabs <= limit and p0.reduce == 0
        elif v.kind == "shards":
            (a0, a1), (b0, b1), (c0, c1) = [p.shard for p in v.parts]
            assert a0 == 0 and a1 == b0 == 1 and b1 == c0 and c1 == v.n_gl * v.n_sph
            assert v.parts[0].n_dirs == 0 and b1 % v.n_sph != 0 and (b1 * sph_eff) % v.n_sph != 0
            assert len({p.n_dirs for p in v.parts}) == 3 and all(p.n_chunks >= 3 for p in v.parts[1:])
        elif v.kind == "batch":
            assert v.max_batch == 3 and v.n_batch == 2 and p0.n_chunks >= 3 and p0.n_dirs % p0.chunk_dirs != 0
        else:
            assert v.merged == 0 and v.n_sph % 2 == 1 and p0.n_dirs == v.n_gl * v.n_sph


def test_plan_in_effective_directions_covers_every_shard_once(oracle):
    """What test_plan_chunks_and_segments_cover_shard_once (tests/test_emu_kernels.py) checks for the faithful mode, with
    the flags set: on every shipped design (antipodal pairs merged: sph_eff = n_sph / 2) and on odd rules (nothing merged),
    n_gl = 1 .. 4, P = 1 .. 8 even shards and seeded random cuts in full directions, max_chunk 0, 1, 3, 7: the ranks'
    effective ranges [floor(b0 sph_eff / n_sph), floor(b1 sph_eff / n_sph)) tile [0, n_gl sph_eff) once, the chunks tile
    each range, the segments tile each chunk in slab order, and no segment straddles a radial node in effective units."""
    rng = np.random.default_rng(20261018)
    rules = [(n, oracle.spherical_design(n), n // 2) for n in (6, 12, 32, 48, 70, 94, 120, 156, 192)]
    rules += [(n, BR.random_rule(n, seed=n), n) for n in (9, 13)]
    checked = 0
    for n_sph, sph, sph_eff in rules:
        for n_gl in (1, 2, 3, 4):
            B = n_gl * n_sph
            cuts = [[(r * (B // P) + min(r, B % P), (r + 1) * (B // P) + min(r + 1, B % P)) for r in range(P)] for P in range(1, 9)]
            for _ in range(2):
                c = sorted({0, B} | {int(x) for x in rng.integers(0, B + 1, size=3)})
                cuts.append(list(zip(c[:-1], c[1:])))
            for flags, nv in ((MC.EXACT, 64), (MC.EXACT | MC.HERMITIAN, 24)):
                for mc in (0, 1, 3, 7):
                    for ranks in cuts:
                        end = 0
                        for b0, b1 in ranks:
                            if (b0, b1) == (0, 0):
                                continue                 # (0, 0) means the whole handle in a descriptor
                            e0, e1 = b0 * sph_eff // n_sph, b1 * sph_eff // n_sph
                            assert e0 == end
                            end = e1
                            chunks, segs = E.plan(nv, n_gl, n_sph, 64, (b0, b1), mc, flags=flags, sph=sph)
                            cap = mc or 1024
                            assert len(chunks) == -(-(e1 - e0) // cap)
                            pos, seg_pos = 0, 0
                            for ci, (n_seg, d0, n, per_group, seg0) in enumerate(chunks):
                                assert d0 == pos and 1 <= n <= cap and seg0 == seg_pos
                                inner = 0
                                for (c, sd0, sn, r) in segs[seg0:seg0 + n_seg]:
                                    assert c == ci and sd0 == inner and sn >= 1
                                    g0, g1 = e0 + d0 + sd0, e0 + d0 + sd0 + sn - 1
                                    assert g0 // sph_eff == r == g1 // sph_eff, (n_sph, n_gl, flags, mc, (b0, b1))
                                    inner += sn
                                assert inner == n
                                pos += n
                                seg_pos += n_seg
                            assert pos == e1 - e0 and seg_pos == len(segs), (n_sph, n_gl, flags, mc, (b0, b1))
                            checked += 1
                        assert end == n_gl * sph_eff
    assert checked > 5000


# ---- the variants of the small sizes under the emulator -----------------------------------------------------------------

def emulate(oracle, v, flags):
    """The variant's calls under the emulator with the given flags; returns the list of its members' Q."""
    inp = MC.inputs(oracle, v.n)
    f, L = inp["f"], inp["L"]
    gl = oracle.gauss_legendre(v.n_gl, 0.0, R)
    sph = MC.rule(oracle, v)
    if v.kind == "batch":
        return list(E.collide_batch(np.stack([f, inp["f1"]]), gl, sph, GAMMA, B_GAMMA, L, v.prec, v.max_chunk, flags,
                                    max_batch=v.max_batch))
    if v.kind in ("many", "noanti") and not v.small:
        # the two-call sequence: the separate Reduce launch, which the library takes above 8 slabs
        return [E.collide(f, gl, sph, GAMMA, B_GAMMA, L, v.prec, max_chunk=v.max_chunk, flags=flags)[0]]
    # bfsm_collide_partial_async: the whole-direction kernels where the handle has them, else the reduce fused into the tail
    total = 0
    for rank, p in enumerate(v.parts):
        total = total + E.collide_partial(f, gl, sph, GAMMA, B_GAMMA, L, v.prec, dir_range=p.shard or (0, 0), with_loss=(rank == 0),
                                          flags=flags, max_chunk=v.max_chunk)
    return [total]


EMU_VARIANTS = [v for v in MC.VARIANTS if v.n in EMU_SIZES]


@pytest.mark.parametrize("v", EMU_VARIANTS, ids=MC.vid)
def test_emulated_variant_matches_oracle(oracle, v):
    """Every variant of N = 16 and 24 (chunks-many, chunks-few, shards with the empty effective shard, batch, no-antipode), both modes,
    both precisions.  fp64: 1e-12 as in tests/test_emu_kernels.py.  fp32: the modes change the rounding order only, so
    they may err twice as much as the emulated faithful mode on the same calls."""
    got = emulate(oracle, v, MC.flags(v))
    errs = [_rel(q, MC.reference(oracle, v, i)) for i, q in enumerate(got)]
    if v.prec == 64:
        print(f"{MC.vid(v)}: max rel err {max(errs):.2e} (bound {TOL64:.0e})")
        assert max(errs) <= TOL64
    else:
        faithful = emulate(oracle, v, MC.flags(v) & ~(MC.EXACT | MC.HERMITIAN))
        base = [_rel(q, MC.reference(oracle, v, i)) for i, q in enumerate(faithful)]
        print(f"{MC.vid(v)}: max rel err {max(errs):.2e}, faithful mode {max(base):.2e}")
        for e, b in zip(errs, base):
            assert e <= 2.0 * b
    if v.kind == "batch":       # a member of a batch is the single call on the same handle, bit for bit
        inp = MC.inputs(oracle, v.n)
        gl = oracle.gauss_legendre(v.n_gl, 0.0, R)
        one = E.collide_batch(inp["f1"][None], gl, MC.rule(oracle, v), GAMMA, B_GAMMA, inp["L"], v.prec, v.max_chunk, MC.flags(v),
                              max_batch=v.max_batch)[0]
        assert np.array_equal(one, got[1])


# ---- each GPU case can fail for the right reason ------------------------------------------------------------------------

def _without_nyquist(f):
    """f with its modes l = -N/2 (index N/2 on any axis) removed; still real."""
    fh = np.fft.fftn(f)
    h = f.shape[0] // 2
    fh[h, :, :] = 0
    fh[:, h, :] = 0
    fh[:, :, h] = 0
    return np.fft.ifftn(fh).real


@pytest.mark.parametrize("n", [pytest.param(n, marks=pytest.mark.slow) if n in (80, 96) else n for n in MC.SIZES])
def test_each_case_can_fail_for_the_right_reason(oracle, n):
    """With the oracle alone, on every distinct reference the GPU module compares against at this size (the design rule's
    whole field, the few-slab shard with the full loss, the second batch member, the odd rule), relative to max|Q_ref| and
    against the looser (fp32) bound of the size's cases: (a) the reference without its last direction lies >= 1000 bounds
    away, so a lost direction, chunk or shard shows; (b) the reference on the input without its Nyquist modes lies >= 100
    bounds away, so the Hermitian mode's Nyquist rows matter."""
    inp = MC.inputs(oracle, n)
    for kind, member in (("many", 0), ("few", 0), ("batch", 1), ("noanti", 0)):
        (v,) = [v for v in MC.VARIANTS if (v.n, v.prec, v.mode, v.kind) == (n, 32, "hermitian", kind) and not v.small]
        gl = oracle.gauss_legendre(v.n_gl, 0.0, R)
        sph = MC.rule(oracle, v)
        ref = MC.reference(oracle, v, member)
        f = inp["f1" if member else "f"]
        b0, b1 = v.parts[0].shard if kind == "few" else (0, v.n_gl * v.n_sph)
        a = _rel(oracle.collide(f, gl, sph, GAMMA, B_GAMMA, inp["L"], dir_range=(b0, b1 - 1)), ref)
        b = _rel(oracle.collide(_without_nyquist(f), gl, sph, GAMMA, B_GAMMA, inp["L"], dir_range=(b0, b1)), ref)
        print(f"N={n} {kind} (member {member}, {v.rule} rule, directions {b0}..{b1}): (a) last direction left out {a:.2e} = "
              f"{a / TOL32:.0f} x fp32 bound, {a / TOL64:.1e} x fp64 bound; (b) Nyquist modes removed {b:.2e} = {b / TOL32:.0f} x "
              f"fp32 bound")
        assert a >= 1000 * TOL32, kind
        assert b >= 100 * TOL32, kind
