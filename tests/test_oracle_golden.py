"""Pins the parity oracle (oracle/) to the reference's own known-answer values.

The reference has no test-suite; its verification is the BKW error-norm printout archived under
Results/ (SURVEY.md section 4).  These tests check the CPU restatement against every such value.
"""
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "bkw_norms.json")))
GAMMA, B_GAMMA, R = 0.0, 1.0 / (4.0 * np.pi), 10.0


def _run(oracle, row):
    f, q_exact, L, dv = oracle.bkw(row["nv"])
    gl = oracle.gauss_legendre(row["n_gl"], 0.0, R)
    sph = oracle.spherical_design(row["n_sph"])
    Q = oracle.collide(f, gl, sph, GAMMA, B_GAMMA, L)
    return Q, oracle.error_norms(Q, q_exact, dv)


def _check(row, norms):
    # the logs print 9 significant digits -> 5e-9 relative; N=64 L1 carries the reference's own
    # atomics-order spread (+-3e-15 on 8.9e-11)
    for name, got in zip(("L1", "L2", "Linf"), norms):
        rtol = row.get(name + "_rtol", 6e-9)
        assert got == pytest.approx(row[name], rel=rtol), (name, got, row)


@pytest.mark.parametrize("row", [r for r in GOLD["published"] if r["nv"] <= 32], ids=lambda r: f"N{r['nv']}_gl{r['n_gl']}_s{r['n_sph']}")
def test_published_norms_n32(oracle, row):
    _, norms = _run(oracle, row)
    _check(row, norms)


@pytest.mark.slow
@pytest.mark.parametrize("row", [r for r in GOLD["published"] if r["nv"] == 64], ids=lambda r: f"N{r['nv']}_gl{r['n_gl']}_s{r['n_sph']}")
def test_published_norms_n64(oracle, row):
    _, norms = _run(oracle, row)
    _check(row, norms)


@pytest.mark.parametrize("row", [r for r in GOLD["survey"] if r["nv"] <= 32], ids=lambda r: f"N{r['nv']}_gl{r['n_gl']}_s{r['n_sph']}")
def test_survey_recorded_values(oracle, row):
    Q, norms = _run(oracle, row)
    _check(row, norms)
    if "sum_abs_Q" in row:
        assert np.abs(Q).sum() == pytest.approx(row["sum_abs_Q"], rel=2e-10)
    if "probe" in row:
        i, j, k, v = row["probe"]
        assert Q[i, j, k] == pytest.approx(v, rel=2e-12)


def test_axis_permutation_equivariance(oracle):
    """Permuting the velocity axes of f together with the components of the quadrature directions permutes Q exactly
    (up to rounding): pins the anisotropic wiring -- which sigma component multiplies which mode index, the layout of
    the 3-D transforms -- that the isotropic BKW norms cannot see.  Also: the order of the directions is immaterial."""
    f, _, L, _ = oracle.bkw(16)
    f = oracle.perturbed_input(f)                      # no symmetry, energy in every Nyquist plane
    gl = oracle.gauss_legendre(3, 0.0, R)
    x, y, z, w = oracle.spherical_design(12)
    # rotate the design first so that no axis permutation maps it onto itself
    a, b = 0.3, 1.1
    x, y = np.cos(a) * x - np.sin(a) * y, np.sin(a) * x + np.cos(a) * y
    y, z = np.cos(b) * y - np.sin(b) * z, np.sin(b) * y + np.cos(b) * z
    sig = np.stack([x, y, z])
    q0 = oracle.collide(f, gl, (x, y, z, w), GAMMA, B_GAMMA, L)
    for perm in ((1, 2, 0), (2, 0, 1), (1, 0, 2), (0, 2, 1), (2, 1, 0)):
        fp = np.ascontiguousarray(f.transpose(perm))               # fp[i0,i1,i2] = f at velocity axes permuted
        sp = sig[list(perm)]
        qp = oracle.collide(fp, gl, (sp[0].copy(), sp[1].copy(), sp[2].copy(), w), GAMMA, B_GAMMA, L)
        assert np.abs(qp - q0.transpose(perm)).max() <= 1e-13 * np.abs(q0).max(), perm
        # the wrong pairing must be visibly different (the check has teeth)
        qbad = oracle.collide(fp, gl, (x, y, z, w), GAMMA, B_GAMMA, L)
        assert np.abs(qbad - q0.transpose(perm)).max() >= 1e-6 * np.abs(q0).max(), perm
    order = np.random.default_rng(3).permutation(12)
    qs = oracle.collide(f, gl, (x[order].copy(), y[order].copy(), z[order].copy(), w[order].copy()), GAMMA, B_GAMMA, L)
    assert np.abs(qs - q0).max() <= 1e-13 * np.abs(q0).max()


def test_c_oracle_matches_numpy_restatement(oracle):
    """Two restatements with unrelated FFTs (own radix-2 vs pocketfft) agree to rounding."""
    f, _, L, _ = oracle.bkw(16)
    gl = oracle.gauss_legendre(8, 0.0, R)
    sph = oracle.spherical_design(32)
    for inp in (f, oracle.perturbed_input(f)):
        qc, hc = oracle.collide(inp, gl, sph, GAMMA, B_GAMMA, L, return_qhat=True)
        qn, hn = oracle.collide_numpy(inp, gl, sph, GAMMA, B_GAMMA, L, return_qhat=True)
        assert np.abs(qc - qn).max() <= 1e-13 * np.abs(qn).max()
        assert np.abs(hc - hn).max() <= 1e-13 * np.abs(hn).max()


def test_direction_shards_sum_to_whole(oracle):
    """Gain term is a plain sum over directions: shards add up (basis of the multi-GPU split)."""
    f, _, L, _ = oracle.bkw(16)
    f = oracle.perturbed_input(f)
    gl = oracle.gauss_legendre(4, 0.0, R)
    sph = oracle.spherical_design(12)
    B = 48
    _, whole = oracle.collide(f, gl, sph, GAMMA, B_GAMMA, L, return_qhat=True)
    parts = sum(oracle.collide(f, gl, sph, GAMMA, B_GAMMA, L, dir_range=(a, b), return_qhat=True)[1]
                for a, b in ((0, 17), (17, 30), (30, B)))
    assert np.abs(parts - whole).max() <= 1e-14 * np.abs(whole).max()


def test_fft_round_trip_and_naive_dft(oracle):
    """fftw_benchmark.cpp:137-171 style round trip + a direct O(n^2) DFT check on a non-cubic box."""
    rng = np.random.default_rng(7)
    a = rng.standard_normal((8, 4, 16)) + 1j * rng.standard_normal((8, 4, 16))
    fw = oracle.fft3d(a, -1)
    assert np.abs(fw - np.fft.fftn(a)).max() < 1e-12
    back = oracle.fft3d(fw, +1) / a.size
    assert np.abs(back - a).sum() < 1e-12
    b = rng.standard_normal((6, 10, 12)) + 0j          # non power-of-two path
    assert np.abs(oracle.fft3d(b, -1) - np.fft.fftn(b)).max() < 1e-11


def test_gauss_legendre_matches_numpy(oracle):
    for n in (1, 2, 3, 8, 16, 30, 32, 64):
        x, w = oracle.gauss_legendre(n, 0.0, 10.0)
        xn, wn = np.polynomial.legendre.leggauss(n)
        assert np.all(np.diff(x) > 0)
        assert np.abs(x - (5 + 5 * xn)).max() < 5e-14
        assert np.abs(w - 5 * wn).max() < 5e-14
        assert w.sum() == pytest.approx(10.0, rel=1e-14)


def test_spherical_designs(oracle):
    """count, unit norm, exact antipodal pairing s <-> s+n/2, weights 4pi/n (SphericalDesign.cpp:48)."""
    for n in (6, 12, 32, 48, 70, 94, 120, 156, 192):
        x, y, z, w = oracle.spherical_design(n)
        assert len(x) == n
        assert np.abs(x * x + y * y + z * z - 1).max() < 1e-15
        h = n // 2
        assert np.array_equal(x[:h], -x[h:]) and np.array_equal(y[:h], -y[h:]) and np.array_equal(z[:h], -z[h:])
        assert np.all(w == 4 * np.pi / n)
    with pytest.raises(ValueError):
        oracle.spherical_design(13)


def test_design_tables_bit_identical_to_reference_data(oracle):
    """Our re-encoded data tables hold exactly the doubles of the reference's ssTTT.NNN.txt files (kept as the data
    fixture tests/golden/ref_sph_designs.npz, see make_fixtures.py)."""
    import re
    ref_tables = np.load(os.path.join(HERE, "golden", "ref_sph_designs.npz"))
    assert sorted(int(re.fullmatch(r"ss\d+\.(\d+)", k).group(1)) for k in ref_tables.files) == \
        [6, 12, 32, 48, 70, 94, 120, 156, 192]
    for key in ref_tables.files:
        n = int(key.split(".")[1])
        ref = ref_tables[key]
        x, y, z, _ = oracle.spherical_design(n)
        assert ref.shape == (n, 3)
        assert np.array_equal(ref, np.stack([x, y, z], axis=1))


def test_oracle_reproduces_committed_q_fixtures(oracle):
    """Data-only regression guard: tests/golden/q_cfg1_*.npy were written by tests/golden/make_fixtures.py."""
    f, _, L, _ = oracle.bkw(16)
    gl = oracle.gauss_legendre(8, 0.0, R)
    sph = oracle.spherical_design(32)
    for name, inp in (("q_cfg1_bkw.npy", f), ("q_cfg1_random.npy", oracle.perturbed_input(f))):
        want = np.load(os.path.join(HERE, "golden", name))
        got = oracle.collide(inp, gl, sph, GAMMA, B_GAMMA, L)
        assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()      # thread count / libm independent


def test_cpu_driver_prints_the_archived_lines(oracle):
    """oracle/maxwell_bkw_oracle: the reference's CPU driver maxwell_bkw_fftw.cpp (BASELINE config 1, "reference
    plumbing") restated over the oracle -- same flags, same report.  Run as `maxwell_bkw_fftw_ex --Nv 32 --Ns 12` its
    error lines are, character for character, those archived in Results/maxwell_bkw_fftw_atomics.txt:19-21; config 1
    itself (--Nv 16 --Ngl 8 --Ns 32) prints the values SURVEY.md 8(c) recorded."""
    import re
    import subprocess
    root = os.path.dirname(HERE)
    subprocess.check_call(["make", "-C", os.path.join(root, "oracle"), "-s"])
    exe = os.path.join(root, "oracle", "maxwell_bkw_oracle")
    ddir = os.path.join(root, "boltzmann-fourier-spectral-method_amd", "data", "sph_design")
    out = subprocess.run([exe, "--Nv", "32", "--Ns", "12", "-t", "2", "--design-dir", ddir], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr
    assert "Run arguments:\nNv = 32\nNs = 12\ntrials = 2" in out.stdout and "Total number of samples taken: 2" in out.stdout
    row = GOLD["published"][0]
    for k in ("L1", "L2", "Linf"):
        assert re.search(k + r" error: (\S+)", out.stdout).group(1) == "%.8e" % row[k]
    out = subprocess.run([exe, "--Nv", "16", "--Ngl", "8", "--Ns", "32", "--design-dir", ddir], capture_output=True, text=True,
                         timeout=600)
    row = [r for r in GOLD["survey"] if r["nv"] == 16 and r["n_gl"] == 8][0]
    for k in ("L1", "L2", "Linf"):
        assert float(re.search(k + r" error: (\S+)", out.stdout).group(1)) == pytest.approx(row[k], rel=6e-9)
