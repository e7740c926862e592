"""Cost of the linearized operator L_f[h] = Q(f,h) + Q(h,f) by the routes the library offers: one process, HIP events around
each route, the routes alternating in the same run; prints one JSON line per workload with the medians over the repeats and
appends it to --out (default profiles/symmetric_rate.jsonl).  No pass / fail gate.

  a  two bfsm_collide_bilinear_async calls + the sum, on a faithful handle (linearizedCollision's work)
  b  bfsm_collide_symmetric_async on a faithful handle
  c  ... on a BFSM_FLAG_EXACT_REDUCTIONS handle
  d  ... on a BFSM_FLAG_EXACT_REDUCTIONS | BFSM_FLAG_HERMITIAN handle
  qa, qd  bfsm_collide_async (Q(f,f)) on the handles of a and d, for scale
Then one profiled call of b, c, d on handles with BFSM_FLAG_PROFILE: the per-kernel times of the symmetric sequence.

usage: python3 tools/symmetric_rate.py [cfg3 cfg2] [--repeats K] [--out FILE]
  cfg3: N = 64 fp64, M_gl = 16, 48-point design;  cfg2: N = 32 fp64, M_gl = 8, 48-point design"""
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

CASES = {"cfg3": dict(nv=64, n_gl=16, n_sph=48), "cfg2": dict(nv=32, n_gl=8, n_sph=48)}


def make(w, mode, profile=False):
    c = bfsm.reference_constants()
    op = bfsm.HIPBoltzmannOperator(bfsm.GaussLegendreQuadrature(w["n_gl"], 0.0, c["R"]), bfsm.SphericalDesign(w["n_sph"]),
                                   w["nv"], w["nv"], w["nv"], c["gamma"], c["b_gamma"], c["L"])
    op.setExactReductions(mode != "faithful", hermitian=(mode == "hermitian"))
    op.setProfiling(profile)
    op.initialize()
    return op


def run(name, repeats):
    w = CASES[name]
    n = w["nv"]
    f_h = bfsm.perturbed_input(bfsm.bkw_solution(n)[0])
    rng = np.random.default_rng(7)
    f = torch.from_numpy(f_h).cuda()
    h = torch.from_numpy(f_h * (rng.random(f_h.shape) - 0.45)).cuda()
    Q, tmp = torch.empty_like(f), torch.empty_like(f)
    ops = {m: make(w, m) for m in ("faithful", "exact", "hermitian")}
    s = torch.cuda.current_stream()
    st = s.cuda_stream

    def route_a():
        ops["faithful"].computeBilinearCollisionAsync(Q, f, h, st)
        ops["faithful"].computeBilinearCollisionAsync(tmp, h, f, st)
        Q.add_(tmp)

    calls = {"a": route_a,
             "b": lambda: ops["faithful"].computeSymmetricCollisionAsync(Q, f, h, st),
             "c": lambda: ops["exact"].computeSymmetricCollisionAsync(Q, f, h, st),
             "d": lambda: ops["hermitian"].computeSymmetricCollisionAsync(Q, f, h, st),
             "qa": lambda: ops["faithful"].computeCollisionAsync(Q, f, st),
             "qd": lambda: ops["hermitian"].computeCollisionAsync(Q, f, st)}
    results = {}
    for k, fn in calls.items():                          # warm-up; the routes must agree on L_f[h]
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        results[k] = Q.clone()
    scale = results["a"].abs().max().item()
    agree = {k: (results[k] - results["a"]).abs().max().item() / scale for k in ("b", "c", "d")}
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
    for op in ops.values():
        op.destroy()
    out = {"case": name, "nv": n, "n_gl": w["n_gl"], "n_sph": w["n_sph"], "repeats": repeats,
           "lib": os.environ.get("BFSM_LIB", "default"), "max_rel_diff_from_a": {k: float("%.3g" % v) for k, v in agree.items()}}
    for k, v in ms.items():
        out["ms_" + k] = round(statistics.median(v), 4)
        out["ms_" + k + "_minmax"] = [round(min(v), 4), round(max(v), 4)]
    out["ratio_d_over_a"] = round(out["ms_d"] / out["ms_a"], 4)
    out["ratio_d_over_qd"] = round(out["ms_d"] / out["ms_qd"], 4)
    out["ratio_b_over_a"] = round(out["ms_b"] / out["ms_a"], 4)
    out["ratio_c_over_a"] = round(out["ms_c"] / out["ms_a"], 4)
    for key, mode in (("b", "faithful"), ("c", "exact"), ("d", "hermitian")):
        op = make(w, mode, profile=True)
        for _ in range(2):
            op.computeSymmetricCollision(Q, f, h)
        cnt = op.counters()
        out["kernel_ms_" + key] = {kn: round(cnt.kernel_ms[i], 4) for i, kn in enumerate(capi.KERNEL_NAMES)}
        out["kernel_launches_" + key] = {kn: cnt.kernel_launches[i] for i, kn in enumerate(capi.KERNEL_NAMES)}
        op.destroy()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats, out = 20, os.path.join(ROOT, "profiles", "symmetric_rate.jsonl")
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
