#!/usr/bin/env python3
"""Regenerates the small Q fixtures of tests/golden/ from the parity oracle (oracle/bfsm_oracle.c).

Provenance: these vectors are produced by the CPU restatement, NOT by the reference (which cannot be built in this
image: FFTW3 / GSL / CUDA are absent).  The restatement itself is pinned by the reference's published BKW norms
(bkw_norms.json).  The fixtures freeze its output so that a later edit of the oracle or of the kernels that changes
results shows up as a diff against committed data, and so that the GPU tests also have a data-only reference.

  q_cfg1_bkw.npy     Q for BASELINE config 1 (N=16, M_gl=8, 32-point design), BKW f at t = 6.5
  q_cfg1_random.npy  same operator, seeded perturbed f (oracle.perturbed_input, seed 0x5EED, amp 0.1)

  ref_sph_designs.npz  the reference's own spherical-design tables (Quadratures/ssTTT.NNN.txt), parsed to doubles, one
                       (NNN, 3) array per file keyed "ssTTT.NNN"; data only, written by
                       `make_fixtures.py --designs <reference checkout>/Quadratures`
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import oracle as O  # noqa: E402


def designs(qdir):
    import glob
    tables = {}
    for p in sorted(glob.glob(os.path.join(qdir, "ss*.txt"))):
        tables[os.path.basename(p)[:-4]] = np.array([[float(v) for v in ln.split()] for ln in open(p) if ln.strip()])
    np.savez(os.path.join(HERE, "ref_sph_designs.npz"), **tables)
    print("written ref_sph_designs.npz", sorted(tables))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--designs":
        return designs(sys.argv[2])
    f, _, L, _ = O.bkw(16)
    gl = O.gauss_legendre(8, 0.0, 10.0)
    sph = O.spherical_design(32)
    args = (gl, sph, 0.0, 1.0 / (4.0 * np.pi), L)
    np.save(os.path.join(HERE, "q_cfg1_bkw.npy"), O.collide(f, *args, threads=1))
    np.save(os.path.join(HERE, "q_cfg1_random.npy"), O.collide(O.perturbed_input(f), *args, threads=1))
    print("written", [n for n in os.listdir(HERE) if n.endswith(".npy")])


if __name__ == "__main__":
    main()
