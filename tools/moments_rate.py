"""Cost of the macroscopic-state calls (bfsm_moments_async, bfsm_maxwellian_async) beside the conservative projection
(bfsm_conserve_async): one handle, HIP events around each call, the three alternating in the same run; prints one JSON line per
case with the medians over the repeats and appends it to --out (default profiles/moments_rate.jsonl).  There is no pass / fail
gate: the figures stand beside the projection's so that a reader sees what the calls cost.

usage: python3 tools/moments_rate.py [cfg3 cfg2 cfg2b64] [--repeats K] [--out FILE]
  cfg3: N = 64, single;  cfg2: N = 32, single;  cfg2b64: N = 32, a batch of 64.  None of the three calls depends on the
  quadrature, so the handles carry a small one (2 x 6 directions)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd"))
import numpy as np
import torch
import bfsm
from bfsm import capi

CASES = {
    "cfg3": dict(shape=(64, 64, 64), batch=1),
    "cfg2": dict(shape=(32, 32, 32), batch=1),
    "cfg2b64": dict(shape=(32, 32, 32), batch=64),
}


def run(name, repeats):
    w = CASES[name]
    nb = w["batch"]
    c = bfsm.reference_constants()
    op = bfsm.HIPBoltzmannOperator(bfsm.GaussLegendreQuadrature(2, 0.0, c["R"]), bfsm.SphericalDesign(6), *w["shape"],
                                   c["gamma"], c["b_gamma"], c["L"])
    if nb > 1:
        op.setMaxBatch(nb)
    op.initialize()
    rng = np.random.default_rng(7)
    f = torch.from_numpy(rng.random((nb,) + w["shape"]) + 0.1).cuda()
    Q = f.clone()
    M = torch.empty_like(f)
    mom = torch.empty(nb, capi.MOM_COUNT, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    calls = {"conserve": lambda: op.conserve(Q, nb, s.cuda_stream),
             "moments": lambda: op.moments(mom, f, nb, s.cuda_stream),
             "maxwellian": lambda: op.maxwellian(M, mom, nb, s.cuda_stream)}
    for _ in range(3):                                   # warm-up of all three
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
    op.destroy()
    out = {"case": name, "shape": list(w["shape"]), "batch": nb, "repeats": repeats, "lib": os.environ.get("BFSM_LIB", "default"),
           "array_bytes": int(f.numel() * 8)}
    for k, v in ms.items():
        out["ms_" + k] = round(statistics.median(v), 4)
        out["ms_" + k + "_minmax"] = [round(min(v), 4), round(max(v), 4)]
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats, out = 50, os.path.join(ROOT, "profiles", "moments_rate.jsonl")
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
        with open(out, "a") as fh:
            fh.write(line + "\n")
