"""What error diffusion under each preset kernel (hq_diffuse_population) costs next to
Floyd-Steinberg's (hq_dither_population; both are instances of diffuse_kernel) in the same run,
and that neither they nor the plain SWASA step moved against the parent commit.

    python scripts/diffusion_timing.py [--parent-lib PATH] [--out profiles/diffusion_unified.json]

Per shape one process (one context) on the synthetic benchmark image: for hq_dither_population
and then for each preset `warmup` untimed and `reps` profiled calls at strength 1 with the same
P random palettes.  The times are HIP events carried by the launches (hq_profile_*, stage
"dither"), medians over the reps with every rep beside them.  Every instance runs one workgroup
per palette, the P workgroups side by side on P CUs: the time per launch is one palette's.  Next
to each time: its ratio to Floyd-Steinberg's and the ratio of the step counts, (W + S H) / (W + 2 H).

--parent-lib: a libhq.so built from the parent commit.  Each shape's process then runs four
times, alternating that library with this tree's (parent, new, new, parent), and per kernel the
table "kernels_vs_parent" holds the process medians, the parent's own spread (the difference of
its two process medians) and whether this tree's median is within the parent's plus that spread.
The plain device-resident C3 step is timed by scripts/repair_timing.py's code in processes of its
own, alternating the same way; all series go to the same file.
"""

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import repair_timing  # noqa: E402

SHAPES = {"C1": (512, 16, 4), "C2": (1024, 64, 1), "C3": (4096, 256, 4)}  # (in the order they run)
FS = "floyd_steinberg"


def child(args):
    import numpy as np
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    size, K, P = SHAPES[args.child]
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    R, G, B = synthetic_planes(size, size, 1)
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), size, size,
                                             _lib.fptr(sp.illuminant), 0, size), m.ctx)
    pals = np.random.default_rng(K).random((P, 4 * K), np.float32)
    pals[:, 3::4] = 0.0
    out = {"shape": args.child, "kernels": {}}
    lib.hq_profile_enable(m.ctx, 1)
    for name in (None,) + _lib.DIFFUSION_PRESETS[1:]:  # (None: hq_dither_population)
        for _ in range(args.warmup):
            costs = m.ditherPopulation(pals, 1.0, 2.0, kernel=name)
        path = m.lastPath()
        reps = []
        for _ in range(args.reps):
            lib.hq_profile_reset(m.ctx)
            m.ditherPopulation(pals, 1.0, 2.0, kernel=name)
            ms, n = C.c_double(), C.c_int64()
            _lib.check(lib.hq_profile_get(m.ctx, b"dither", C.byref(ms), C.byref(n)), m.ctx)
            reps.append(ms.value / n.value)
        S = path["diffuse_slope"] or 2
        out["kernels"][name or FS] = {
            "argmin": path["argmin"], "rows": path["diffuse_rows"], "slope": path["diffuse_slope"],
            "ms_per_palette": round(statistics.median(reps), 5), "ms_per_palette_reps": [round(x, 5) for x in reps],
            "steps_over_floyd_steinberg": round((size + S * size) / (size + 2 * size), 4),
            "mean_cost": float(np.mean(costs))}
    m.close()
    base = out["kernels"][FS]["ms_per_palette"]
    for v in out["kernels"].values():
        v["time_over_floyd_steinberg"] = round(v["ms_per_palette"] / base, 4)
    print("RESULT " + json.dumps(out))


def run_self(args, *extra, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps), *extra]
    env = dict(os.environ, HQ_LIB_PATH=os.path.abspath(lib)) if lib else None
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls before the profiled ones")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (plain C3 step, A/B)")
    ap.add_argument("--step-iters", type=int, default=200, help="A/B: iterations per hq_search_run call")
    ap.add_argument("--step-reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusion_unified.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    out = {"shapes": {k: f"{v[0]}x{v[0]}, K={v[1]}, P={v[2]}" for k, v in SHAPES.items()},
           "warmup_calls": args.warmup, "reps": args.reps,
           "statistic": "median over reps of the HIP-event time of the launch under stage 'dither' of hq_profile_*; "
                        "a launch runs its P workgroups side by side, one palette each"}
    for shape in SHAPES:
        if not args.parent_lib:
            out[shape] = run_self(args, "--child", shape)
            print(shape, json.dumps(out[shape]), flush=True)
            continue
        runs = {"parent": [], "new": []}
        for name in ("parent", "new", "new", "parent"):
            runs[name].append(run_self(args, "--child", shape, lib=args.parent_lib if name == "parent" else None))
        out[shape] = runs["new"][0]
        table = {}
        for k in out[shape]["kernels"]:
            reps = {n: [r["kernels"][k]["ms_per_palette_reps"] for r in rs] for n, rs in runs.items()}
            pm = {n: [round(statistics.median(x), 5) for x in v] for n, v in reps.items()}
            med = {n: statistics.median(x for run in v for x in run) for n, v in reps.items()}
            spread = abs(pm["parent"][0] - pm["parent"][1])
            table[k] = {"ms_per_palette_reps": reps, "process_medians_ms": pm,
                        "median_ms": {n: round(v, 5) for n, v in med.items()},
                        "parent_spread_ms": round(spread, 5), "new_minus_parent_ms": round(med["new"] - med["parent"], 5),
                        "within_parent_spread": med["new"] <= med["parent"] + spread,
                        "mean_cost_equal": len({r["kernels"][k]["mean_cost"] for rs in runs.values() for r in rs}) == 1}
        out[shape]["kernels_vs_parent"] = table
        print(shape, json.dumps(table), flush=True)
    if args.parent_lib:
        step = argparse.Namespace(iters=args.step_iters, warmup=3, reps=args.step_reps, prof_reps=1, timeout=args.timeout)
        ab = {"parent": [], "new": []}
        for name in ("parent", "new", "new", "parent"):
            lib = args.parent_lib if name == "parent" else None
            res = repair_timing.run_child(step, "C3", lib, plain_only=True)
            ab[name].append(res["device_plain"]["ms_per_iteration_reps"])
        med = {k: statistics.median(x for run in v for x in run) for k, v in ab.items()}
        pm = {k: [statistics.median(run) for run in v] for k, v in ab.items()}
        out["plain_step_vs_parent"] = {
            "shape": "C3, device-resident plain search, host clock around hq_search_run / iterations",
            "iterations_per_call": args.step_iters, "ms_per_iteration_reps": ab,
            "median_ms": {k: round(v, 5) for k, v in med.items()},
            "process_medians_ms": {k: [round(x, 5) for x in v] for k, v in pm.items()},
            "new_minus_parent_ms": round(med["new"] - med["parent"], 5),
            "spread_between_process_medians_ms": {k: round(abs(v[0] - v[1]), 5) for k, v in pm.items()},
            "new_over_parent": round(med["new"] / med["parent"], 4)}
        print(json.dumps(out["plain_step_vs_parent"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
