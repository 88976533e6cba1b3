"""What the dither kernel (hq_dither_population) costs next to the grid, assign and cost
kernels of a plain evaluation, and that the plain SWASA step did not move.

    python scripts/dither_timing.py [--parent-lib PATH] [--out profiles/dither_c3.json]

Per shape one process (one context) on the synthetic benchmark image: `warmup` untimed and
`reps` profiled calls of hq_eval_population, then the same of hq_dither_population at
strength 1, with the same P random palettes.  The times are HIP events carried by the
launches (hq_profile_*), medians over the reps with every rep beside them.  The dither
kernel runs one workgroup per palette, the P workgroups side by side on P CUs: its time per
launch is one palette's time for every P up to the CU count, and is reported as such.

Then one observation, no gate: on a 128 x 128 benchmark image (K = 8, P = 3, 60 iterations)
the cost of the dithered rendering of the plain search's palette against the cost a
dither-aware search (findBestQuantization ditherSearch=True) ends with.

--parent-lib: a libhq.so built from the parent commit.  Its plain device-resident C3 step
is timed by scripts/repair_timing.py's code in processes of its own, alternating with this
tree's (parent, new, new, parent); both series go to the same file.
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
# A kernel of many seconds is no good neighbour on a shared device: C3 runs only if C2's time
# times 32 (8 times the steps, 4 times the colours) stays below this
C3_LIMIT_MS = 20000.0
KERNELS = ("dither", "grid", "assign", "cost", "finalize")


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
    out = {"shape": args.child}
    lib.hq_profile_enable(m.ctx, 1)
    calls = {"plain": lambda: m.computeQuantizationErrorPopulation(pals, 2.0),
             "dithered": lambda: m.ditherPopulation(pals, 1.0, 2.0)}
    for name, call in calls.items():
        for _ in range(args.warmup):
            costs = call()
        kern = {k: [] for k in KERNELS}
        for _ in range(args.reps):
            lib.hq_profile_reset(m.ctx)
            call()
            for k in KERNELS:
                ms, n = C.c_double(), C.c_int64()
                _lib.check(lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n)), m.ctx)
                if n.value:
                    kern[k].append(ms.value / n.value)
        out[name] = {"costs": [float(v) for v in costs],
                     "kernel_ms_per_launch": {k: round(statistics.median(v), 5) for k, v in kern.items() if v},
                     "kernel_ms_per_launch_reps": {k: [round(x, 5) for x in v] for k, v in kern.items() if v}}
    m.close()
    d, p = out["dithered"]["kernel_ms_per_launch"], out["plain"]["kernel_ms_per_launch"]
    out["dither_ms_per_palette"] = d["dither"]
    out["plain_ms_per_palette"] = {k: round(p[k] / P, 5) for k in ("grid", "assign", "cost")}
    out["dither_ns_per_pixel_and_colour"] = round(d["dither"] * 1e6 / (size * size * K), 4)
    print("RESULT " + json.dumps(out))


def search_observation():
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd.scielab_processor import makeinline

    import numpy as np

    w, K, P, iters = 128, 8, 3, 60
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    rgba = makeinline(np.stack(synthetic_planes(w, w, 1)))
    out = {"image": f"{w}x{w} benchmark image", "K": K, "P": P, "iterations": iters, "seed": 17}
    for name, kw in (("plain_search_then_dither", dict(dither=1.0)),
                     ("dither_search", dict(dither=1.0, ditherSearch=True)),
                     ("mediancut_plain_search_then_dither", dict(dither=1.0, init="mediancut")),
                     ("mediancut_dither_search", dict(dither=1.0, ditherSearch=True, init="mediancut"))):
        sw = hq.SWASA(population=P, imax=iters, seed=17)
        m.findBestQuantization(rgba, None, w, K, sw, None, None, sp.illuminant, iterations=iters, **kw)
        out[name] = {"bestError": m.bestError, "bestErrorDithered": m.bestErrorDithered}
    m.close()
    print("RESULT " + json.dumps(out))


def run_self(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dither_c3.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--observe", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    if args.observe:
        return search_observation()
    out = {"shapes": {k: f"{v[0]}x{v[0]}, K={v[1]}, P={v[2]}" for k, v in SHAPES.items()},
           "warmup_calls": args.warmup, "reps": args.reps,
           "statistic": "median over reps of the HIP-event time of each kernel's launch under hq_profile_*; the "
                        "dither kernel's launch runs its P workgroups side by side, one palette each"}
    for shape in SHAPES:
        if shape == "C3" and out["C2"]["dither_ms_per_palette"] * 32 > C3_LIMIT_MS:
            out[shape] = {"skipped": f"C2 took {out['C2']['dither_ms_per_palette']} ms: 32 times that is too long"}
            continue
        out[shape] = run_self(args, "--child", shape)
        print(shape, json.dumps(out[shape]), flush=True)
    out["dither_search_observation"] = run_self(args, "--observe")
    print(json.dumps(out["dither_search_observation"]), flush=True)
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
