"""Time Q(f,f) (bfsm_collide_async) against the bilinear Q(g,f) (bfsm_collide_bilinear_async) in one process, with HIP
events around each call, the two alternating; prints one JSON line per case with the medians over the repeats.

usage: python3 tools/bilinear_rate.py [cfg3] [cfg5] [--repeats K]
  cfg3: N = 64, 16 x 48 directions, fp64;  cfg5: N = 128, 30 x 192 directions (the full rule), fp32."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd"))
import numpy as np
import torch
import bfsm

CASES = {"cfg3": dict(nv=64, n_gl=16, n_sph=48, precision=64), "cfg5": dict(nv=128, n_gl=30, n_sph=192, precision=32)}


def run(name, repeats):
    w = CASES[name]
    nv, n_gl, n_sph, prec = w["nv"], w["n_gl"], w["n_sph"], w["precision"]
    c = bfsm.reference_constants()
    op = bfsm.HIPBoltzmannOperator(bfsm.GaussLegendreQuadrature(n_gl, 0.0, c["R"]), bfsm.SphericalDesign(n_sph),
                                   nv, nv, nv, c["gamma"], c["b_gamma"], c["L"])
    op.setPrecision(prec)
    op.initialize()
    f0 = bfsm.bkw_solution(nv)[0]
    f = torch.from_numpy(bfsm.perturbed_input(f0)).cuda()
    g = torch.from_numpy(bfsm.perturbed_input(f0, seed=0xB11)).cuda()
    Q = torch.empty_like(f)
    s = torch.cuda.current_stream()
    calls = {"ff": lambda: op.computeCollisionAsync(Q, f, s.cuda_stream),
             "gf": lambda: op.computeBilinearCollisionAsync(Q, g, f, s.cuda_stream)}
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
    op.destroy()
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"case": name, "nv": nv, "n_gl": n_gl, "n_sph": n_sph, "precision": prec, "repeats": repeats,
                      "ms_Qff": round(med["ff"], 4), "ms_Qgf": round(med["gf"], 4),
                      "ratio": round(med["gf"] / med["ff"], 4),
                      "ms_Qff_minmax": [round(min(ms["ff"]), 4), round(max(ms["ff"]), 4)],
                      "ms_Qgf_minmax": [round(min(ms["gf"]), 4), round(max(ms["gf"]), 4)]}), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats = 20
    if "--repeats" in args:
        i = args.index("--repeats")
        repeats = int(args[i + 1])
        del args[i:i + 2]
    for name in args or ["cfg3", "cfg5"]:
        run(name, repeats)
