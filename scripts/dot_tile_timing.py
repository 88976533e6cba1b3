"""What dot diffusion's tiled form (hq_dot_tile.hip: one launch, a window per workgroup, errors
in LDS) costs next to the chain of one launch per class (hq_dot.hip), in the same process and
alternating, and that the plain SWASA step did not move against the parent commit.

    python scripts/dot_tile_timing.py [--parent-lib PATH] [--parent-tree DIR] [--out profiles/dot_tile_c3.json]

Per shape one process (one context) on the synthetic benchmark image, the method of
scripts/dot_timing.py: for P = 1 and P = 4 random palettes and for Knuth's matrix and one
16 x 16 permutation, `warmup` untimed rounds and `reps` profiled ones; a round is one call of
hq_dot_population at strength 1 under "dot_tile" 0 (the chain) and one under "dot_tile" 1 with
each tile shape ("dot_tile_shape" 1, 2, 3), in that order.  Recorded per call: the HIP-event time
of the "dot" stage (the chain: from the first launch's start to the last one's end; the tiled
form: its one launch) and the host's wall time around the call.  Medians over the reps, every rep
beside them, and the chain's own spread (largest minus smallest rep): the tiled form counts as
faster at a shape only when its median beats the chain's by more than that spread.  Both forms'
costs are compared as doubles on the way.  Then, in one more process, the device-resident
search at C3 under the dot-diffused cost with each form, the plain step beside it.

--parent-lib: a libhq.so built from the parent commit.  The plain device-resident C3 step is
then timed by scripts/repair_timing.py's code in four processes alternating that library with
this tree's (parent, new, new, parent); the two-sided rule: |difference of the medians| within
the larger spread between the two process medians of one library.

--parent-tree: a checkout of the parent commit with its library built.  bench.py as it stands is
then run in it and in this tree alternately (parent, new, parent, new), one process each, and the
four ms_per_step figures are recorded.
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
from dot_timing import _context  # noqa: E402

# (in the order they run; C0 is the small end of what option "dot_tile" -1 takes)
SHAPES = {"C0": (128, 16), "C1": (512, 16), "C2": (1024, 64), "C3": (4096, 256)}

PS = (1, 4)
FORMS = (("chain", 0, 0), ("tile_16x16", 1, 1), ("tile_32x32", 1, 2), ("tile_64x32", 1, 3))


def _dot_ms(m):
    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    ms, n = C.c_double(), C.c_int64()
    _lib.check(hq.load().hq_profile_get(m.ctx, b"dot", C.byref(ms), C.byref(n)), m.ctx)
    assert n.value == 1
    return round(ms.value, 5)


def child_shape(args):
    import numpy as np

    import hybridquantization_amd as hq

    lib = hq.load()
    size, K = SHAPES[args.child]
    m, _ = _context(size)
    matrices = {"knuth8": None, "perm16": np.random.default_rng(46).permutation(256).astype(np.int32).reshape(16, 16)}
    out = {"shape": args.child, "size": size, "K": K, "cases": {}}
    lib.hq_profile_enable(m.ctx, 1)
    for mname, cls in matrices.items():
        for P in PS:
            pals = np.random.default_rng(K).random((P, 4 * K), np.float32)
            pals[:, 3::4] = 0.0
            stage = {f[0]: [] for f in FORMS}
            wall = {f[0]: [] for f in FORMS}
            form_seen, costs = {}, {}
            for rep in range(args.warmup + args.reps):
                for name, tile, shape in FORMS:
                    m.setOption("dot_tile", tile)
                    m.setOption("dot_tile_shape", shape)
                    lib.hq_profile_reset(m.ctx)
                    t0 = time.perf_counter()
                    c = m.dotPopulation(pals, 1.0, 2.0, classes=cls)
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep >= args.warmup:
                        stage[name].append(_dot_ms(m))
                        wall[name].append(round(dt, 4))
                    form_seen[name], costs[name] = m.dotForm(), [float(x) for x in c]
            row = {"reach": list(hq.ImageManipulation.dotReach2(cls)), "levels": form_seen["chain"][3]}
            for name, _, _ in FORMS:
                row[name] = {"form": list(form_seen[name]), "stage_ms": round(statistics.median(stage[name]), 5),
                             "stage_ms_reps": stage[name], "wall_ms": round(statistics.median(wall[name]), 4),
                             "wall_ms_reps": wall[name], "costs_equal_chain": costs[name] == costs["chain"]}
            spread = max(stage["chain"]) - min(stage["chain"])
            row["chain_spread_ms"] = round(spread, 5)
            for name, _, _ in FORMS[1:]:
                row[name]["chain_over_tiled"] = round(row["chain"]["stage_ms"] / row[name]["stage_ms"], 3)
                row[name]["faster_by_more_than_chain_spread"] = \
                    row["chain"]["stage_ms"] - row[name]["stage_ms"] > spread
            out["cases"][f"{mname} P={P}"] = row
    m.close()
    print("RESULT " + json.dumps(out))


def child_search(args):
    """ms per iteration of the device-resident search at C3 (4096^2, K = 256, P = 4): the plain
    step, then the search under the dot-diffused cost (hq_search_set_dot, Knuth's matrix, strength
    1) with the chain and with the tiled kernel, in one process; the host clock around
    hq_search_run over its iterations."""
    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    size, K = SHAPES["C3"]
    m, _ = _context(size)
    out = {"shape": "C3", "size": size, "K": K, "P": 4, "iterations_per_call": args.search_iters, "modes": {}}
    for mode, tile in (("plain", None), ("dot_chain", 0), ("dot_tiled_64x32", 1), ("plain_again", None)):
        if tile is not None:
            m.setOption("dot_tile", tile)
            m.setOption("dot_tile_shape", 0)
        sw = hq.SWASA(population=4, imax=10 ** 7, seed=1)
        params, h = sw.params(), C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, sw.seed, C.byref(h)), m.ctx)
        try:
            if tile is not None:
                _lib.check(lib.hq_search_set_dot(h, None, 1.0), m.ctx)
            ran, reps = C.c_int(), []
            _lib.check(lib.hq_search_run(h, 3, C.byref(ran)), m.ctx)  # (warm-up)
            for _ in range(args.reps):
                t0 = time.perf_counter()
                _lib.check(lib.hq_search_run(h, args.search_iters, C.byref(ran)), m.ctx)
                reps.append(round((time.perf_counter() - t0) * 1e3 / ran.value, 5))
            err = C.c_double()
            _lib.check(lib.hq_search_best(h, None, C.byref(err), None), m.ctx)
            out["modes"][mode] = {"ms_per_iteration": round(statistics.median(reps), 5), "ms_per_iteration_reps": reps,
                                  "dot_form": list(m.dotForm()), "argmin": m.lastPath()["argmin"],
                                  "best_error": err.value}
        finally:
            lib.hq_search_destroy(h)
    m.close()
    print("RESULT " + json.dumps(out))


def run_self(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps),
           "--search-iters", str(args.search_iters), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1, help="untimed rounds before the profiled ones")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (plain C3 step, A/B)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (bench.py, A/B)")
    ap.add_argument("--step-iters", type=int, default=200, help="A/B: iterations per hq_search_run call")
    ap.add_argument("--step-reps", type=int, default=9)
    ap.add_argument("--search-iters", type=int, default=25, help="the dot search: iterations per hq_search_run call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dot_tile_c3.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "search":
        return child_search(args)
    if args.child is not None:
        return child_shape(args)
    out = {"shapes": {k: f"{v[0]}x{v[0]}, K={v[1]}, P in {list(PS)}" for k, v in SHAPES.items()},
           "warmup_rounds": args.warmup, "reps": args.reps,
           "statistic": "median over reps of the 'dot' stage (HIP events carried by the launches); a round runs the "
                        "chain, then the tiled form under each tile shape; chain_spread_ms: the chain's largest minus "
                        "smallest rep in that process",
           "not_measured": "more than one GPU"}
    for shape in SHAPES:
        out[shape] = run_self(args, "--child", shape)
        print(shape, json.dumps(out[shape]), flush=True)
    out["search"] = run_self(args, "--child", "search")
    print("search", json.dumps(out["search"]), flush=True)
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
    if args.parent_tree:
        runs = {"parent": [], "new": []}
        for name in ("parent", "new", "parent", "new"):
            cwd = os.path.abspath(args.parent_tree) if name == "parent" else ROOT
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=cwd,
                               capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:
                raise RuntimeError(f"bench.py in {cwd} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
            res = json.loads(r.stdout.strip().splitlines()[-1])
            runs[name].append(res["ms_per_step"])
            print("bench.py", name, res["ms_per_step"], flush=True)
        lo, hi = min(runs["parent"]), max(runs["parent"])
        out["bench_py_vs_parent"] = {
            "command": "bench.py --gpus 1 --steps 200 --warmup 20, one process per run, parent and new alternating",
            "ms_per_step": runs, "new_within_parents_runs": all(lo <= x <= hi for x in runs["new"])}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
