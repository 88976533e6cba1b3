"""What pattern dithering (hq_pattern.hip) costs and what it buys, next to the other renderings, in
one process per shape and alternating.

    python scripts/pattern_timing.py [--ab NAME=LIB ...] [--parent-tree DIR] [--out profiles/pattern_c3.json]

Time.  Per shape one process (one context) on the synthetic benchmark image, the method of
scripts/dot_tile_timing.py: for P = 1 and P = 4 random palettes, `warmup` untimed rounds and `reps`
profiled ones; a round is one call each of hq_pattern_population (n = 16, strength 1), hq_ordered_population,
hq_dot_population and hq_dither_population, in that order.  Recorded per call: the HIP-event time of the
stage that makes the index images ("pattern", "assign", "dot", "dither"), medians over the reps with
every rep beside them.  The yardstick is arithmetic: n K distances per pixel at 10 VALU instructions each
(3 differences, a product, 2 fma, a compare, 2 selects, a median) against the FP32 vector peak taken as
157.3 TFLOP/s / 2 lane-instructions per second (DESIGN.md 8's peak; an fma counts two there).

--ab NAME=LIB: the "pattern" stage alone, timed the same way with another build of the library (the
pixels-per-lane A/B: make BUILD=build_px2 EXTRA=-DHQ_PATTERN_PX=2 OUT=../libhq_px2.so), in processes
alternating with this tree's.

Quality.  One more process: the cost on the 64 x 64 ramp under the eight cube corners and on the 128 x 128
benchmark noise image at K = 16 (scripts/assign_space_timing.py's palette seed), for the nearest colour,
ordered dithering at orderedAmplitude(K), Floyd-Steinberg, dot diffusion and pattern dithering at n = 16
and 64, strength 1.

--parent-tree: a built checkout of the parent commit: bench.py there and here alternately, one process each.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from dot_timing import _context  # noqa: E402

SHAPES = {"C1": (512, 16), "C2": (1024, 64), "C3": (4096, 256)}
PS = (1, 4)
N = 16
PEAK_LANE_INSTR = 157.3e12 / 2
INSTR_PER_DISTANCE = 10


def _stage_ms(m, name):
    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    ms, n = C.c_double(), C.c_int64()
    _lib.check(hq.load().hq_profile_get(m.ctx, name.encode(), C.byref(ms), C.byref(n)), m.ctx)
    assert n.value == 1, (name, n.value)
    return round(ms.value, 5)


def child_shape(args):
    import numpy as np

    import hybridquantization_amd as hq

    lib = hq.load()
    size, K = SHAPES[args.child]
    m, _ = _context(size)
    amp = hq.ImageManipulation.orderedAmplitude(K)
    calls = [("pattern", "pattern", lambda p: m.patternPopulation(p, N, 1.0, 2.0))]
    if not args.pattern_only:
        calls += [("ordered", "assign", lambda p: m.orderedPopulation(p, amp, 2.0)),
                  ("dot", "dot", lambda p: m.dotPopulation(p, 1.0, 2.0)),
                  ("dither", "dither", lambda p: m.ditherPopulation(p, 1.0, 2.0))]
    out = {"shape": args.child, "size": size, "K": K, "n": N, "lib": os.environ.get("HQ_LIB_PATH", "this tree"), "P": {}}
    lib.hq_profile_enable(m.ctx, 1)
    for P in PS:
        pals = np.random.default_rng(K).random((P, 4 * K), np.float32)
        pals[:, 3::4] = 0.0
        reps = {c[0]: [] for c in calls}
        for rep in range(args.warmup + args.reps):
            for name, stage, call in calls:
                lib.hq_profile_reset(m.ctx)
                call(pals)
                if rep >= args.warmup:
                    reps[name].append(_stage_ms(m, stage))
        row = {name: {"stage_ms": round(statistics.median(v), 5), "stage_ms_reps": v} for name, v in reps.items()}
        least = N * K * size * size * P * INSTR_PER_DISTANCE / PEAK_LANE_INSTR * 1e3
        row["pattern"]["least_ms_at_valu_peak"] = round(least, 5)
        row["pattern"]["fraction_of_valu_peak"] = round(least / row["pattern"]["stage_ms"], 4)
        out["P"][str(P)] = row
    m.close()
    print("RESULT " + json.dumps(out))


def child_quality(args):
    import numpy as np

    import hybridquantization_amd as hq
    from assign_space_timing import noise_image
    from dither_ref import cube_corners, ramp_image

    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    rgba, n = noise_image(128)
    images = {"ramp64_cube_corners": (ramp_image(64, 64), 64, cube_corners().reshape(1, -1).astype(np.float32)),
              "noise128_k16": (rgba, n, None)}
    out = {}
    for name, (img, w, pal) in images.items():
        if pal is None:
            pal = np.random.default_rng(16).random((1, 64), np.float32)
            pal[:, 3::4] = 0.0
        K = pal.shape[1] // 4
        m.setImage(np.asarray(img, np.float32).reshape(-1), None, w, sp.illuminant)
        amp = hq.ImageManipulation.orderedAmplitude(K)
        cost = {"nearest": m.computeQuantizationErrorPopulation(pal, 0.0)[0],
                "ordered": m.orderedPopulation(pal, amp, 0.0)[0],
                "floyd_steinberg": m.ditherPopulation(pal, 1.0, 0.0)[0],
                "dot": m.dotPopulation(pal, 1.0, 0.0)[0],
                "pattern_n16": m.patternPopulation(pal, 16, 1.0, 0.0)[0],
                "pattern_n64": m.patternPopulation(pal, 64, 1.0, 0.0)[0]}
        out[name] = {"K": K, "ordered_amplitude": amp, "mean_dE": {k: float(v) for k, v in cost.items()},
                     "over_nearest": {k: round(float(v / cost["nearest"]), 4) for k, v in cost.items()}}
    m.close()
    print("RESULT " + json.dumps(out))


def run_self(args, *extra, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps), *extra]
    env = dict(os.environ, **({"HQ_LIB_PATH": os.path.abspath(lib)} if lib else {}))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--ab", action="append", default=[], help="NAME=LIB: another build's pattern stage, alternating")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (bench.py, A/B)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern_c3.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--pattern-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "quality":
        return child_quality(args)
    if args.child is not None:
        return child_shape(args)
    out = {"statistic": "median over reps of the stage's HIP-event time (the events ride on the launches); a round "
                        "runs pattern, ordered, dot, dither in that order; warm-up rounds untimed",
           "warmup_rounds": args.warmup, "reps": args.reps, "n": N,
           "valu_yardstick": f"n K pixels P x {INSTR_PER_DISTANCE} lane-instructions over {PEAK_LANE_INSTR:.4g} per second",
           "not_measured": "more than one GPU; a register sorting network in the place of the counting selection"}
    out["quality"] = run_self(args, "--child", "quality")
    print("quality", json.dumps(out["quality"]), flush=True)
    for shape in SHAPES:
        out[shape] = run_self(args, "--child", shape)
        print(shape, json.dumps(out[shape]), flush=True)
    if args.ab:
        builds = [("this_tree", None)] + [tuple(x.split("=", 1)) for x in args.ab]
        ab = {name: [] for name, _ in builds}
        for name, lib in builds + builds[::-1]:  # (alternating: each build first once and last once)
            res = run_self(args, "--child", "C3", "--pattern-only", lib=lib)
            ab[name].append({P: res["P"][P]["pattern"]["stage_ms_reps"] for P in res["P"]})
            print("A/B", name, json.dumps(ab[name][-1]), flush=True)
        out["pixels_per_lane_ab_C3"] = {
            name: {"runs": runs, "median_ms": {P: round(statistics.median(x for r in runs for x in r[P]), 5)
                                               for P in runs[0]}} for name, runs in ab.items()}
    if args.parent_tree:
        runs = {"parent": [], "new": []}
        for name in ("parent", "new", "parent", "new"):
            cwd = os.path.abspath(args.parent_tree) if name == "parent" else ROOT
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=cwd,
                               capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py in {cwd} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
            print("bench.py", name, runs[name][-1], flush=True)
        lo, hi = min(runs["parent"]), max(runs["parent"])
        out["bench_py_vs_parent"] = {
            "command": "bench.py --gpus 1 --steps 200 --warmup 20, one process per run, parent and new alternating",
            "ms_per_step": runs, "new_within_parents_runs": all(lo <= x <= hi for x in runs["new"])}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
