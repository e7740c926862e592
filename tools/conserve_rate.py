"""Cost of the conservative projection (BFSM_FLAG_CONSERVE): one handle without and one with the flag, the same input, HIP
events around each evaluation, the two alternating; prints one JSON line per case with the medians over the repeats
(and appends it to --out when given).

usage: python3 tools/conserve_rate.py [cfg1 cfg1b64 cfg2 cfg3 cfg5 gen] [--repeats K] [--out FILE]
  cfg1: N = 16, 8 x 32 directions (single evaluation: the whole-direction kernels);  cfg1b64: the same, a batch of 64;
  cfg2: N = 32, 8 x 48;  cfg3: N = 64, 16 x 48;  cfg5: N = 128, 30 x 192, fp32;  gen: a 60 x 48 x 40 box (size-generic
  path), 8 x 48.  BFSM_LIB selects another build of the library (e.g. another BFSM_CONS_SMALL_G)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd"))
import numpy as np
import torch
import bfsm

CASES = {
    "cfg1": dict(shape=(16, 16, 16), n_gl=8, n_sph=32, precision=64, batch=1),
    "cfg1b64": dict(shape=(16, 16, 16), n_gl=8, n_sph=32, precision=64, batch=64),
    "cfg2": dict(shape=(32, 32, 32), n_gl=8, n_sph=48, precision=64, batch=1),
    "cfg3": dict(shape=(64, 64, 64), n_gl=16, n_sph=48, precision=64, batch=1),
    "cfg5": dict(shape=(128, 128, 128), n_gl=30, n_sph=192, precision=32, batch=1),
    "gen": dict(shape=(60, 48, 40), n_gl=8, n_sph=48, precision=64, batch=1),
}


def _handle(w, conserve):
    c = bfsm.reference_constants()
    op = bfsm.HIPBoltzmannOperator(bfsm.GaussLegendreQuadrature(w["n_gl"], 0.0, c["R"]), bfsm.SphericalDesign(w["n_sph"]),
                                   *w["shape"], c["gamma"], c["b_gamma"], c["L"])
    op.setPrecision(w["precision"])
    op.setConservation(conserve)
    if w["batch"] > 1:
        op.setMaxBatch(w["batch"])
    op.initialize()
    return op


def run(name, repeats):
    w = CASES[name]
    nb = w["batch"]
    ops = {"off": _handle(w, False), "on": _handle(w, True)}
    rng = np.random.default_rng(7)
    f = torch.from_numpy(rng.random((nb,) + w["shape"]) + 0.1).cuda()
    Q = torch.empty_like(f)
    s = torch.cuda.current_stream()
    if nb > 1:
        calls = {k: (lambda op=op: op.computeCollisionBatch(Q, f, nb, s.cuda_stream)) for k, op in ops.items()}
    else:
        calls = {k: (lambda op=op: op.computeCollisionAsync(Q[0], f[0], s.cuda_stream)) for k, op in ops.items()}
    for _ in range(3):                                   # warm-up of both
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    for op in ops.values():
        op.destroy()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"case": name, "shape": list(w["shape"]), "n_gl": w["n_gl"], "n_sph": w["n_sph"], "precision": w["precision"],
            "batch": nb, "repeats": repeats, "lib": os.environ.get("BFSM_LIB", "default"),
            "ms_off": round(med["off"], 4), "ms_on": round(med["on"], 4),
            "overhead": round(med["on"] / med["off"] - 1.0, 4),
            "ms_off_minmax": [round(min(ms["off"]), 4), round(max(ms["off"]), 4)],
            "ms_on_minmax": [round(min(ms["on"]), 4), round(max(ms["on"]), 4)]}


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats, out = 20, None
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
        line = json.dumps(run(name, repeats))
        print(line, flush=True)
        if out:
            with open(out, "a") as fh:
                fh.write(line + "\n")
