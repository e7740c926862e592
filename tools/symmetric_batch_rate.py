"""Cost of the batched symmetric form against the loop it replaces: bfsm_collide_symmetric_batch_partial_async for n_batch pairs
against n_batch bfsm_collide_symmetric_async calls ON THE SAME HANDLE (max_batch 32), one process, HIP events around each route,
the two routes alternating in the same run; per grid one exact + Hermitian and one faithful handle, n_batch = 1, 8, 32,
BFSM_SHARE_NONE and BFSM_SHARE_F.  Prints one JSON line per (grid, mode) with the medians over the repeats and appends it to --out
(default profiles/symmetric_batch_rate.jsonl).  No pass / fail gate.

max_chunk bounds the A' scratch of the 32-member handle to about 40 GB (it bounds scratch, not results; both routes run the same
chunks).  ratio = ms_batch / ms_loop: below 1 the batch wins.

usage: python3 tools/symmetric_batch_rate.py [cfg1 cfg2 cfg3] [--repeats K] [--out FILE]
  cfg1: N = 16 fp64, M_gl = 8, 32-point design;  cfg2: N = 32, M_gl = 8, 48 points;  cfg3: N = 64, M_gl = 16, 48 points"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd"))
import numpy as np
import torch
import bfsm

CASES = {"cfg1": dict(nv=16, n_gl=8, n_sph=32), "cfg2": dict(nv=32, n_gl=8, n_sph=48), "cfg3": dict(nv=64, n_gl=16, n_sph=48)}
MAX_BATCH = 32
BATCHES = (1, 8, 32)
SCRATCH_BYTES = 40e9


def make(w, mode):
    c = bfsm.reference_constants()
    n = w["nv"]
    planes = n // 2 + 1 if mode == "hermitian" else n
    chunk = int(SCRATCH_BYTES / (MAX_BATCH * planes * n * n * 16 * 2))
    op = bfsm.HIPBoltzmannOperator(bfsm.GaussLegendreQuadrature(w["n_gl"], 0.0, c["R"]), bfsm.SphericalDesign(w["n_sph"]),
                                   n, n, n, c["gamma"], c["b_gamma"], c["L"])
    op.setExactReductions(mode != "faithful", hermitian=(mode == "hermitian"))
    op.setMaxBatch(MAX_BATCH)
    op.setMaxChunk(min(chunk, 1024))
    op.initialize()
    return op


def run(name, mode, repeats):
    w = CASES[name]
    n = w["nv"]
    f_h = bfsm.perturbed_input(bfsm.bkw_solution(n)[0])
    rng = np.random.default_rng(7)
    f = torch.from_numpy(np.stack([f_h * (1.0 + 0.01 * i) for i in range(MAX_BATCH)])).cuda()
    h = torch.from_numpy(np.stack([f_h * (rng.random(f_h.shape) - 0.45) for _ in range(MAX_BATCH)])).cuda()
    Q, Q1 = torch.empty_like(f), torch.empty_like(f)
    op = make(w, mode)
    s = torch.cuda.current_stream()
    st = s.cuda_stream
    out = {"case": name, "mode": mode, "nv": n, "n_gl": w["n_gl"], "n_sph": w["n_sph"], "max_batch": MAX_BATCH, "repeats": repeats,
           "n_chunks": op.counters().n_chunks, "lib": os.environ.get("BFSM_LIB", "default")}
    for share in (None, "f"):
        for nb in BATCHES:
            fop = f[0] if share == "f" else f[:nb]

            def batch():
                op.collideSymmetricBatchPartial(Q[:nb], h[:nb], fop, nb, True, share, st)

            def loop():
                for i in range(nb):
                    op.computeSymmetricCollisionAsync(Q1[i], h[i], f[0] if share == "f" else f[i], st)

            calls = {"batch": batch, "loop": loop}
            for fn in calls.values():                      # warm-up; the two routes must agree bit for bit
                fn()
            torch.cuda.synchronize()
            equal = bool(torch.equal(Q[:nb], Q1[:nb]))
            ms = {k: [] for k in calls}
            order = list(calls)
            for r in range(repeats):
                for k in (order if r % 2 == 0 else order[::-1]):        # alternating order
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    calls[k]()
                    e1.record(s)
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1))
            key = f"share_{share or 'none'}_nb{nb}"
            mb, ml = statistics.median(ms["batch"]), statistics.median(ms["loop"])
            out[key] = {"ms_batch": round(mb, 4), "ms_loop": round(ml, 4), "ratio": round(mb / ml, 4), "bitwise_equal": equal,
                        "ms_batch_minmax": [round(min(ms["batch"]), 4), round(max(ms["batch"]), 4)],
                        "ms_loop_minmax": [round(min(ms["loop"]), 4), round(max(ms["loop"]), 4)],
                        "pairs_per_s_batch": round(1e3 * nb / mb, 1), "pairs_per_s_loop": round(1e3 * nb / ml, 1)}
    op.destroy()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats, out = 9, os.path.join(ROOT, "profiles", "symmetric_batch_rate.jsonl")
    if "--repeats" in args:
        i = args.index("--repeats")
        repeats = int(args[i + 1])
        del args[i:i + 2]
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    if repeats < 5:
        sys.exit("--repeats must be at least 5")
    for name in args or list(CASES):
        for mode in ("hermitian", "faithful"):
            line = json.dumps(run(name, mode, repeats))
            print(line, flush=True)
            with open(out, "a") as fh:
                fh.write(line + "\n")
