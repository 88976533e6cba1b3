"""What dot diffusion (hq_dot_population: one launch per class, all CUs) costs next to raster
Floyd-Steinberg (hq_dither_population: one workgroup per palette) in the same process of the
same library, what both renderings cost in S-CIELAB, and that the plain SWASA step did not move
against the parent commit.

    python scripts/dot_timing.py [--parent-lib PATH] [--out profiles/dot_c3.json]

Per shape one process (one context) on the synthetic benchmark image, the method of
scripts/diffusion_timing.py: for P = 1 and P = 4 random palettes, `warmup` untimed and `reps`
profiled calls at strength 1 of hq_dot_population (Knuth's 8 x 8 matrix, 64 launches) and of
hq_dither_population.  Recorded per call: the HIP-event time of the stage ("dot": from the first
launch's start to the last one's end; "dither": the one launch), the host's wall time around
the call, and the stage table of the dot call (dot, cost, finalize).  Medians over the reps,
every rep beside them.  A dither launch runs its P workgroups side by side, so its time hardly
depends on P; the dot launches share the whole device among the P palettes.

The costs: both renderings' S-CIELAB cost (mean dE76 + 2 per unused colour) on the 64 x 64 ramp
under the eight cube corners and on the benchmark image at 512 x 512 under a random 16-colour
palette, next to the nearest-colour cost.

--parent-lib: a libhq.so built from the parent commit.  The plain device-resident C3 step is
then timed by scripts/repair_timing.py's code in four processes alternating that library with
this tree's (parent, new, new, parent); the two-sided rule: |difference of the medians| within
the larger spread between the two process medians of one library.
"""

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import repair_timing  # noqa: E402

SHAPES = {"C1": (512, 16), "C2": (1024, 64), "C3": (4096, 256)}  # (in the order they run)
PS = (1, 4)
STAGES = ("dot", "dither", "grid", "assign", "cost", "finalize")


def _context(size):
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    R, G, B = synthetic_planes(size, size, 1)
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), size, size,
                                             _lib.fptr(sp.illuminant), 0, size), m.ctx)
    m.w = m.h = size  # (what setImage would have noted: getIndices sizes its output by them)
    return m, sp


def _stages(m):
    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib, got = hq.load(), {}
    for k in STAGES:
        ms, n = C.c_double(), C.c_int64()
        _lib.check(lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n)), m.ctx)
        if n.value:
            got[k] = round(ms.value, 5)
    return got


def child_shape(args):
    import numpy as np

    import hybridquantization_amd as hq

    lib = hq.load()
    size, K = SHAPES[args.child]
    m, _ = _context(size)
    out = {"shape": args.child, "size": size, "K": K, "P": {}}
    lib.hq_profile_enable(m.ctx, 1)
    for P in PS:
        pals = np.random.default_rng(K).random((P, 4 * K), np.float32)
        pals[:, 3::4] = 0.0
        row = {}
        for name, call in (("dot", lambda: m.dotPopulation(pals, 1.0, 2.0)),
                           ("dither", lambda: m.ditherPopulation(pals, 1.0, 2.0))):
            for _ in range(args.warmup):
                costs = call()
            stage, wall, tables = [], [], []
            for _ in range(args.reps):
                lib.hq_profile_reset(m.ctx)
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
                tab = _stages(m)
                stage.append(tab[name])
                tables.append(tab)
            row[name] = {"argmin": m.lastPath()["argmin"], "stage_ms": round(statistics.median(stage), 5),
                         "stage_ms_reps": stage, "wall_ms": round(statistics.median(wall), 4),
                         "wall_ms_reps": [round(x, 4) for x in wall], "stages_ms_last_rep": tables[-1],
                         "mean_cost": float(np.mean(costs))}
        row["dither_over_dot_stage"] = round(row["dither"]["stage_ms"] / row["dot"]["stage_ms"], 3)
        row["dither_over_dot_wall"] = round(row["dither"]["wall_ms"] / row["dot"]["wall_ms"], 3)
        out["P"][str(P)] = row
    m.close()
    print("RESULT " + json.dumps(out))


def child_costs(args):
    import numpy as np

    import hybridquantization_amd as hq

    out = {}
    # the 64 x 64 ramp (R along x, G along y, B along the diagonal, k/255) under the cube corners
    w = h = 64
    x, y = np.arange(w)[None, :].repeat(h, 0), np.arange(h)[:, None].repeat(w, 1)
    by = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y) * 255) // (w + h - 2)], -1)
    ramp = np.zeros((w * h, 4), np.float32)
    ramp[:, :3] = by.reshape(-1, 3).astype(np.float32) / np.float32(255)
    corners = np.zeros((8, 4), np.float32)
    for k in range(8):
        corners[k, :3] = [(k >> 2) & 1, (k >> 1) & 1, k & 1]
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.setImage(ramp.reshape(-1), None, w, sp.illuminant)

    def costs(pal):
        pal = pal.reshape(1, -1)
        plain = float(m.computeQuantizationErrorPopulation(pal, 2.0)[0])
        got = {"nearest": plain, "floyd_steinberg": float(m.ditherPopulation(pal, 1.0, 2.0)[0]),
               "dot_1": float(m.dotPopulation(pal, 1.0, 2.0)[0]), "dot_0.5": float(m.dotPopulation(pal, 0.5, 2.0)[0])}
        got["over_nearest"] = {k: round(v / plain, 4) for k, v in got.items() if k != "nearest"}
        return got

    out["ramp_64x64_cube_corners"] = costs(corners)
    m.close()
    m, _ = _context(512)
    pal = np.random.default_rng(16).random((1, 64), np.float32)
    pal[:, 3::4] = 0.0
    out["benchmark_image_512x512_K16"] = costs(pal)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dot_c3.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "costs":
        return child_costs(args)
    if args.child is not None:
        return child_shape(args)
    out = {"shapes": {k: f"{v[0]}x{v[0]}, K={v[1]}, P in {list(PS)}" for k, v in SHAPES.items()},
           "warmup_calls": args.warmup, "reps": args.reps,
           "statistic": "median over reps; stage_ms: HIP events carried by the launches (hq_profile_*: 'dot' from "
                        "the first of the 64 launches' start to the last one's end, 'dither' the one launch, whose P "
                        "workgroups run side by side); wall_ms: the host clock around the whole call"}
    for shape in SHAPES:
        out[shape] = run_self(args, "--child", shape)
        print(shape, json.dumps(out[shape]), flush=True)
    out["costs"] = run_self(args, "--child", "costs")
    print("costs", json.dumps(out["costs"]), flush=True)
    if args.parent_lib:
        step = argparse.Namespace(iters=args.step_iters, warmup=3, reps=args.step_reps, prof_reps=1, timeout=args.timeout)
        ab = {"parent": [], "new": []}
        for name in ("parent", "new", "new", "parent"):
            lib = args.parent_lib if name == "parent" else None
            res = repair_timing.run_child(step, "C3", lib, plain_only=True)
            ab[name].append(res["device_plain"]["ms_per_iteration_reps"])
            print("plain step", name, round(statistics.median(ab[name][-1]), 5), flush=True)
        med = {k: statistics.median(x for run in v for x in run) for k, v in ab.items()}
        pm = {k: [statistics.median(run) for run in v] for k, v in ab.items()}
        spread = {k: abs(v[0] - v[1]) for k, v in pm.items()}
        out["plain_step_vs_parent"] = {
            "shape": "C3, device-resident plain search, host clock around hq_search_run / iterations",
            "iterations_per_call": args.step_iters, "ms_per_iteration_reps": ab,
            "median_ms": {k: round(v, 5) for k, v in med.items()},
            "process_medians_ms": {k: [round(x, 5) for x in v] for k, v in pm.items()},
            "new_minus_parent_ms": round(med["new"] - med["parent"], 5),
            "spread_between_process_medians_ms": {k: round(v, 5) for k, v in spread.items()},
            "within_spread_two_sided": abs(med["new"] - med["parent"]) <= max(spread.values()),
            "new_over_parent": round(med["new"] / med["parent"], 4)}
        print(json.dumps(out["plain_step_vs_parent"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
