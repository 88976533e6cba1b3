"""What fixed palette colours (hq_set_fixed_colors) cost at C3, that the search step with nothing
set did not move, and one quality example.

    python scripts/fixed_timing.py [--parent-lib PATH] [--out profiles/fixed_c3.json]

The method is scripts/weights_timing.py's, whose step child this runs.  C3 (4096^2, K = 256,
P = 4, dE76) on the synthetic benchmark image, device-resident search; a host clock around
hq_search_run, HIP-event stages under hq_profile_*, medians of `reps` after untimed warm-up calls.

--parent-lib: a libhq.so built from the parent commit.  Its C3 step is timed in processes of its
own alternating with this tree's, nothing set (parent, new, new, parent); each new process median
is accepted when it lies within the parent's own process-to-process spread of its neighbouring
parent median.

fixed: one process, one context, bracketed: nothing set, 16 fixed colours, nothing set again --
the plain step, and per launch the `sa_step`, `lloyd` and `reseed` stages of a search whose
every iteration is a hybrid and a repair iteration.

quality: the test blob image (96 x 64, 5 Gaussian blobs), K = 8, population 3, seed 17,
lloydEvery = 1, 60 iterations: the free search, the search with black and white fixed, and the
free search's best palette with its colours nearest to black and to white replaced by them --
what a caller can do without the feature.
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

import mask_timing  # noqa: E402
import weights_timing  # noqa: E402
from mask_timing import K, P, SIZE  # noqa: E402

NFIXED = 16
STAGES = ("sa_step", "lloyd", "reseed")


def _measure(args, hq, _lib, lib, m):
    """The plain step (host clock), then the stages of a search with both moves in every iteration."""
    params = hq.SWASA(population=P, imax=10 ** 7, seed=1).params()
    ran = C.c_int()

    def create():
        h = C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, 1, C.byref(h)), m.ctx)
        return h

    h = create()

    def run():
        t0 = time.perf_counter()
        _lib.check(lib.hq_search_run(h, args.step_iters, C.byref(ran)), m.ctx)
        dt = time.perf_counter() - t0
        assert ran.value == args.step_iters
        return dt * 1e3 / args.step_iters

    for _ in range(args.step_warmup):
        run()
    reps = [run() for _ in range(args.step_reps)]
    best = (C.c_float * (4 * K))()
    _lib.check(lib.hq_search_best(h, best, None, None), m.ctx)
    lib.hq_search_destroy(h)
    h = create()
    _lib.check(lib.hq_search_set_lloyd(h, 1), m.ctx)
    _lib.check(lib.hq_search_set_repair(h, 1, -1), m.ctx)
    lib.hq_profile_enable(m.ctx, 1)
    stage = {k: [] for k in STAGES}
    for i in range(args.warmup + args.reps):
        lib.hq_profile_reset(m.ctx)
        _lib.check(lib.hq_search_run(h, args.move_iters, C.byref(ran)), m.ctx)
        for k in STAGES:
            ms, n = C.c_double(), C.c_int64()
            _lib.check(lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n)), m.ctx)
            if i >= args.warmup and n.value:
                stage[k].append(ms.value / n.value)
    lib.hq_profile_enable(m.ctx, 0)
    lib.hq_search_destroy(h)
    return {"fixed_colours": int(m.fixedColors().shape[0]), "best_first_colour": [float(v) for v in best[:3]],
            "step_ms_per_iteration": round(statistics.median(reps), 5),
            "step_ms_per_iteration_reps": [round(v, 5) for v in reps],
            "stage_ms_per_launch": {k: round(statistics.median(v), 5) for k, v in stage.items() if v},
            "stage_ms_per_launch_reps": {k: [round(x, 5) for x in v] for k, v in stage.items() if v}}


def child_fixed(args):
    import numpy as np

    hq, _lib, lib, m = mask_timing._context()
    fixed = np.random.default_rng(NFIXED).integers(0, 256, (NFIXED, 3)).astype(np.float32) / np.float32(255)
    out = {}
    for name in ("nothing", f"fixed_{NFIXED}", "nothing_again"):
        m.setFixedColors(fixed if name.startswith("fixed") else None)
        out[name] = _measure(args, hq, _lib, lib, m)
    m.close()
    assert out[f"fixed_{NFIXED}"]["best_first_colour"] == [float(v) for v in fixed[0]]
    print("RESULT " + json.dumps(out))


def child_quality(args):
    import numpy as np

    import hybridquantization_amd as hq

    w, h, Kq = 96, 64, 8
    rng = np.random.default_rng(11)  # tests/test_lloyd_gpu.py's blob_image(96, 64, seed=11)
    centres = rng.integers(40, 216, (5, 3))
    which = rng.integers(0, 5, w * h)
    by = np.clip(np.rint(centres[which] + 12.0 * rng.standard_normal((w * h, 3))), 0, 255)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    bw = np.array([[0, 0, 0], [1, 1, 1]], np.float32)

    def search(**kw):
        sw = hq.SWASA(population=3, imax=60, seed=17)
        best = m.findBestQuantization(rgba.reshape(-1), None, w, Kq, sw, None, None, sp.illuminant, iterations=60,
                                      lloydEvery=1, **kw)
        return np.asarray(best, np.float32).reshape(Kq, 4), m.bestError, sw.delta

    free, e_free, delta = search()
    fixed, e_fixed, _ = search(fixed=bw)
    # what a caller can do without the feature: the free palette's colour nearest to black becomes
    # black, then the nearest to white among the others becomes white
    patched = free.copy()
    k_black = int(np.argmin(((patched[:, :3] - bw[0]) ** 2).sum(1)))
    d_white = ((patched[:, :3] - bw[1]) ** 2).sum(1)
    d_white[k_black] = np.inf
    k_white = int(np.argmin(d_white))
    patched[k_black, :3], patched[k_white, :3] = bw[0], bw[1]
    costs, used = m.computeQuantizationErrorPopulation(np.stack([free, fixed, patched]).reshape(3, -1), delta,
                                                       return_used=True)
    m.close()
    print("RESULT " + json.dumps({
        "image": "blob_image(96, 64, seed=11): 5 Gaussian colour blobs",
        "settings": "K=8, population 3, seed 17, lloydEvery=1, 60 iterations, delta %g" % delta,
        "cost_free_search": float(costs[0]), "cost_search_with_black_and_white_fixed": float(costs[1]),
        "cost_free_palette_with_two_colours_replaced": float(costs[2]),
        "used_colours": [int(u.sum()) for u in used],
        "replaced": [k_black, k_white], "search_best_error_free": e_free, "search_best_error_fixed": e_fixed}))


def run_self(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps),
           "--step-iters", str(args.step_iters), "--step-warmup", str(args.step_warmup),
           "--step-reps", str(args.step_reps), "--move-iters", str(args.move_iters), *extra]
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
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (the C3 step with nothing set, A/B)")
    ap.add_argument("--step-iters", type=int, default=200, help="iterations per hq_search_run call")
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=9)
    ap.add_argument("--move-iters", type=int, default=20, help="iterations per profiled call with both moves on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixed_c3.json"))
    ap.add_argument("--child", default=None, choices=("step", "fixed", "quality"), help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--map", default="nothing", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return {"step": weights_timing.child_step, "fixed": child_fixed, "quality": child_quality}[args.child](args)
    out = {"shape": f"C3: {SIZE}x{SIZE}, K={K}, P={P}, dE76, 72 dpi / 45 cm",
           "warmup_calls": args.warmup, "reps": args.reps,
           "statistic": "the search step: median over reps of the host time of hq_search_run / iterations; stages: "
                        "median over reps of the HIP-event time per launch under hq_profile_*",
           "not_measured": "anything on more than one GPU; chunked palettes (K > 256)"}
    # (figures made outside this script -- the disassembly diff, an earlier run's A/B kept by hand -- stay)
    if os.path.exists(args.out):
        with open(args.out) as f:
            out.update({k: v for k, v in json.load(f).items() if k in ("disassembly", "resources", "build", "earlier_runs")})
    if args.parent_lib:  # first, on a fresh device
        ab = {"parent": [], "new": []}
        for name in ("parent", "new", "new", "parent"):
            extra = ["--lib", os.path.abspath(args.parent_lib)] if name == "parent" else []
            ab[name].append(run_self(args, "--child", "step", *extra)["ms_per_iteration_reps"])
        pm = {k: [statistics.median(run) for run in v] for k, v in ab.items()}
        floor = abs(pm["parent"][0] - pm["parent"][1])
        out["plain_step_vs_parent"] = {
            "shape": "C3, packed image, device-resident search, nothing set, host clock around hq_search_run / iterations",
            "order": "parent, new, new, parent", "iterations_per_call": args.step_iters,
            "warmup_calls": args.step_warmup, "ms_per_iteration_reps": ab,
            "process_medians_ms": {k: [round(x, 5) for x in v] for k, v in pm.items()},
            "parent_spread_ms": round(floor, 5),
            "accepted": bool(all(abs(n - p) <= floor for n, p in zip(pm["new"], pm["parent"]))),
            # (beside the rule, not in its place: which side of the parent a new median outside the spread lies on)
            "new_minus_parent_ms": [round(n - p, 5) for n, p in zip(pm["new"], pm["parent"])]}
        print("plain_step_vs_parent", json.dumps({k: out["plain_step_vs_parent"][k] for k in
                                                  ("process_medians_ms", "parent_spread_ms", "accepted", "new_minus_parent_ms")}), flush=True)
    out["fixed_vs_nothing"] = run_self(args, "--child", "fixed")
    print("fixed_vs_nothing", json.dumps({k: (v["step_ms_per_iteration"], v["stage_ms_per_launch"])
                                          for k, v in out["fixed_vs_nothing"].items()}), flush=True)
    out["quality"] = run_self(args, "--child", "quality")
    print("quality", json.dumps(out["quality"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
