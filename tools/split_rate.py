"""Time bfsm_collide_async against the gain / loss split bfsm_collide_split_async on one handle in one process, with HIP
events around each call, the two alternating; one JSON line per case with the medians over the repeats and the min - max of
each, appended to profiles/split_rate.jsonl (BFSM_LIB: time another build of the library; its line is tagged with the path's
file name and, where that build lacks the split, carries the combined call alone).

usage: python3 tools/split_rate.py [cfg3] [cfg2] [--repeats K] [--out FILE]
  cfg3: N = 64, 16 x 48 directions, fp64;  cfg2: N = 32, 8 x 48 directions, fp64."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "boltzmann-fourier-spectral-method_amd"))
import torch
import bfsm

CASES = {"cfg3": dict(nv=64, n_gl=16, n_sph=48, precision=64), "cfg2": dict(nv=32, n_gl=8, n_sph=48, precision=64)}


def run(name, repeats, out):
    w = CASES[name]
    nv, n_gl, n_sph, prec = w["nv"], w["n_gl"], w["n_sph"], w["precision"]
    c = bfsm.reference_constants()
    op = bfsm.HIPBoltzmannOperator(bfsm.GaussLegendreQuadrature(n_gl, 0.0, c["R"]), bfsm.SphericalDesign(n_sph),
                                   nv, nv, nv, c["gamma"], c["b_gamma"], c["L"])
    op.setPrecision(prec)
    op.initialize()
    f = torch.from_numpy(bfsm.perturbed_input(bfsm.bkw_solution(nv)[0])).cuda()
    Q, Qg, nu = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
    s = torch.cuda.current_stream()
    calls = {"collide": lambda: op.computeCollisionAsync(Q, f, s.cuda_stream)}
    if hasattr(op._lib, "bfsm_collide_split_async"):
        calls["split"] = lambda: op.computeCollisionSplitAsync(Qg, nu, f, s.cuda_stream)
    for _ in range(5):                                   # warm-up of both
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
    rec = {"case": name, "nv": nv, "n_gl": n_gl, "n_sph": n_sph, "precision": prec, "repeats": repeats,
           "library": os.path.basename(os.environ.get("BFSM_LIB", "libbfsm_hip.so"))}
    for k, v in ms.items():
        rec["ms_" + k] = round(statistics.median(v), 4)
        rec["ms_" + k + "_minmax"] = [round(min(v), 4), round(max(v), 4)]
    if "split" in ms:
        rec["ratio_split_over_collide"] = round(rec["ms_split"] / rec["ms_collide"], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats = 20
    out = os.path.join(ROOT, "profiles", "split_rate.jsonl")
    for flag in ("--repeats", "--out"):
        if flag in args:
            i = args.index(flag)
            if flag == "--repeats":
                repeats = int(args[i + 1])
            else:
                out = args[i + 1]
            del args[i:i + 2]
    for name in args or ["cfg3", "cfg2"]:
        run(name, repeats, out)
