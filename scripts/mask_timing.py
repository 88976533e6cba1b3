"""What the pixel mask (hq_set_mask) costs and what its tile skip buys at C3, and that the
plain step did not move.

    python scripts/mask_timing.py [--parent-lib PATH] [--out profiles/mask_c3.json]

The method is scripts/ordered_timing.py's.  C3 (4096^2, K = 256, P = 4, dE76) on the synthetic
benchmark image, the packed 8-bit image form.

read: one process, one context.  Without a mask, then under an all-ones mask with option
"mask_skip" 0 (every tile launched: the price of the mask read alone), then without a mask
again: `warmup` untimed and `reps` profiled rounds of hq_eval_population, hq_cluster_sums and
hq_color_histogram (the `cost`, `centroid` and `hist` stages: HIP events carried by the
launches, hq_profile_*), and the device-resident search step (`step-warmup` untimed
hq_search_run calls of `step-iters` iterations and `step-reps` timed ones, a host clock around
the call, profiling off), medians with every rep beside them.

skip: one process per region, a centred square of 1/4 and of 1/16 of the area: the same `cost`
stage and search step with "mask_skip" 1 against 0, and the tiles launched (hq_mask_info).

--parent-lib: a libhq.so built from the parent commit.  Its plain device-resident C3 step is
timed by scripts/repair_timing.py's code in processes of its own, alternating with this tree's
(parent, new, new, parent), 2 warm-up calls and 9 timed ones of 200 iterations each; the new
tree's process medians are accepted when they differ from the parent's by no more than the
parent's own two differ from each other.
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

SIZE, K, P = 4096, 256, 4  # C3
STAGES = ("cost", "centroid", "hist")


def _context():
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    R, G, B = synthetic_planes(SIZE, SIZE, 1)
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), SIZE, SIZE,
                                             _lib.fptr(sp.illuminant), 0, SIZE), m.ctx)
    m.w = m.h = SIZE
    return hq, _lib, lib, m


def _measure(args, hq, _lib, lib, m, pals):
    """The stages of an evaluation, the sums and the histogram, then the search step, under the
    mask and options in force."""
    lib.hq_profile_enable(m.ctx, 1)
    stage = {k: [] for k in STAGES}
    for i in range(args.warmup + args.reps):
        lib.hq_profile_reset(m.ctx)
        costs = m.computeQuantizationErrorPopulation(pals, 2.0)
        m.clusterSums(P, K)
        m.colorHistogram(5)
        for k in STAGES:
            ms, n = C.c_double(), C.c_int64()
            _lib.check(lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n)), m.ctx)
            if i >= args.warmup and n.value:
                stage[k].append(ms.value / n.value)
    info = m.maskInfo()
    lib.hq_profile_enable(m.ctx, 0)
    params = hq.SWASA(population=P, imax=10 ** 7, seed=1).params()
    h, ran = C.c_void_p(), C.c_int()
    _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, 1, C.byref(h)), m.ctx)

    def run():
        t0 = time.perf_counter()
        _lib.check(lib.hq_search_run(h, args.step_iters, C.byref(ran)), m.ctx)
        dt = time.perf_counter() - t0
        assert ran.value == args.step_iters
        return dt * 1e3 / args.step_iters

    for _ in range(args.step_warmup):
        run()
    reps = [run() for _ in range(args.step_reps)]
    lib.hq_search_destroy(h)
    return {"costs": [float(v) for v in costs], "n_full": info[0], "tiles_run": info[2], "tiles_all": info[3],
            "stage_ms_per_launch": {k: round(statistics.median(v), 5) for k, v in stage.items() if v},
            "stage_ms_per_launch_reps": {k: [round(x, 5) for x in v] for k, v in stage.items() if v},
            "step_ms_per_iteration": round(statistics.median(reps), 5),
            "step_ms_per_iteration_reps": [round(v, 5) for v in reps]}


def _palettes():
    import numpy as np

    pals = np.random.default_rng(K).random((P, 4 * K), np.float32)
    pals[:, 3::4] = 0.0
    return pals


def child_read(args):
    import numpy as np

    hq, _lib, lib, m = _context()
    pals, out = _palettes(), {}
    for name in ("plain", "all_ones_no_skip", "plain_again"):
        m.setMask(np.ones((SIZE, SIZE), np.uint8) if name == "all_ones_no_skip" else None)
        m.setOption("mask_skip", 0 if name == "all_ones_no_skip" else 1)
        out[name] = _measure(args, hq, _lib, lib, m, pals)
    m.close()
    assert out["plain"]["costs"] == out["all_ones_no_skip"]["costs"]  # bit for bit
    print("RESULT " + json.dumps(out))


def child_skip(args):
    import numpy as np

    hq, _lib, lib, m = _context()
    side = int(round(SIZE / args.root))  # a centred square of 1 / root^2 of the area
    lo = (SIZE - side) // 2
    mask = np.zeros((SIZE, SIZE), np.uint8)
    mask[lo:lo + side, lo:lo + side] = 1
    m.setMask(mask)
    pals, out = _palettes(), {"region": f"rows and columns [{lo}, {lo + side})", "area_fraction": side * side / SIZE ** 2}
    for skip in (1, 0, 1):
        m.setOption("mask_skip", skip)
        out[f"mask_skip_{skip}" + ("_again" if f"mask_skip_{skip}" in out else "")] = _measure(args, hq, _lib, lib, m, pals)
    m.close()
    assert out["mask_skip_1"]["costs"] == out["mask_skip_0"]["costs"]  # bit for bit
    print("RESULT " + json.dumps(out))


def run_self(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps),
           "--step-iters", str(args.step_iters), "--step-warmup", str(args.step_warmup),
           "--step-reps", str(args.step_reps), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds before the profiled ones")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (plain C3 step, A/B)")
    ap.add_argument("--step-iters", type=int, default=200, help="iterations per hq_search_run call")
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_c3.json"))
    ap.add_argument("--child", default=None, choices=("read", "skip"), help=argparse.SUPPRESS)
    ap.add_argument("--root", type=int, default=2, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "read":
        return child_read(args)
    if args.child == "skip":
        return child_skip(args)
    out = {"shape": f"C3: {SIZE}x{SIZE}, K={K}, P={P}, dE76, 72 dpi / 45 cm, packed 8-bit image",
           "warmup_calls": args.warmup, "reps": args.reps,
           "statistic": "median over reps of the HIP-event time of each stage's launch under hq_profile_*; the "
                        "search step: median over reps of the host time of hq_search_run / iterations",
           "not_measured": "anything on more than one GPU"}
    if args.parent_lib:  # first, on a fresh device
        step = argparse.Namespace(iters=args.step_iters, warmup=args.step_warmup, reps=args.step_reps, prof_reps=1,
                                  timeout=args.timeout)
        ab = {"parent": [], "new": []}
        for name in ("parent", "new", "new", "parent"):
            lib = args.parent_lib if name == "parent" else None
            res = repair_timing.run_child(step, "C3", lib, plain_only=True)
            ab[name].append(res["device_plain"]["ms_per_iteration_reps"])
        pm = {k: [statistics.median(run) for run in v] for k, v in ab.items()}
        floor = abs(pm["parent"][0] - pm["parent"][1])
        lo, hi = min(pm["parent"]) - floor, max(pm["parent"]) + floor
        out["plain_step_vs_parent"] = {
            "shape": "C3, device-resident plain search, host clock around hq_search_run / iterations",
            "order": "parent, new, new, parent", "iterations_per_call": args.step_iters,
            "warmup_calls": args.step_warmup, "ms_per_iteration_reps": ab,
            "process_medians_ms": {k: [round(x, 5) for x in v] for k, v in pm.items()},
            "noise_floor_ms": round(floor, 5),
            "accepted": bool(all(lo <= x <= hi for x in pm["new"]))}
        print(json.dumps(out["plain_step_vs_parent"]), flush=True)
    out["mask_read"] = run_self(args, "--child", "read")
    print(json.dumps({k: (v["stage_ms_per_launch"], v["step_ms_per_iteration"]) for k, v in out["mask_read"].items()}),
          flush=True)
    for root, key in ((2, "region_quarter"), (4, "region_sixteenth")):
        out[key] = run_self(args, "--child", "skip", "--root", str(root))
        print(key, json.dumps({k: (v["tiles_run"], v["tiles_all"], v["stage_ms_per_launch"]["cost"],
                                   v["step_ms_per_iteration"]) for k, v in out[key].items() if isinstance(v, dict)}),
              flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
