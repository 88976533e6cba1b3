"""What a repair iteration (hq_search_set_repair, every = 1) costs next to a plain
SWASA iteration and next to a hybrid one (hq_search_set_lloyd), device-resident and
host-driven, at C3 (4096^2, K = 256, P = 4) and C2 (1024^2, K = 64, P = 1).

    python scripts/repair_timing.py [--parent-lib PATH] [--out profiles/repair_c3.json]

The method is scripts/hybrid_timing.py's.  Per shape one process (one library, one
context), five searches one after the other on the synthetic benchmark image:
device-resident plain, repair and hybrid, host-driven plain and repair.  Each runs
`warmup` untimed hq_search_run calls of `iters` iterations, then `reps` timed ones
(a host clock around the call, which ends in a stream synchronise) with profiling
off, then `prof_reps` more under hq_profile_* for the per-kernel times (HIP events
carried by the launches).  Medians are reported with every repetition beside them.
A repair iteration launches the cost kernel twice, once with the error image
stored: that pass's time is the repair search's "cost" less the plain search's.

--parent-lib: a libhq.so built from the parent commit.  Its plain device-resident
step is timed by the same code in processes of its own, alternating with this
tree's (parent, new, new, parent); the difference of the medians is reported next
to the spread between the process medians of one library.
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

from hybrid_timing import load_lib  # noqa: E402

SHAPES = {"C3": (4096, 256, 4), "C2": (1024, 64, 1)}
KERNELS = ("sa_step", "grid", "assign", "cost", "errsum", "reseed", "centroid", "lloyd")
# mode: (option sa_device, repair every, lloyd every)
MODES = {"device_plain": (1, 0, 0), "device_repair": (1, 1, 0), "device_hybrid": (1, 0, 1),
         "host_plain": (0, 0, 0), "host_repair": (0, 1, 0)}


def child(args):
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = load_lib(args.lib) if args.lib else hq.load()
    size, K, P = SHAPES[args.child]
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    R, G, B = synthetic_planes(size, size, 1)
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), size, size,
                                             _lib.fptr(sp.illuminant), 0, size), m.ctx)
    out = {"shape": args.child, "lib": args.lib or "this tree"}
    for mode in (["device_plain"] if args.plain_only else list(MODES)):
        device, repair, lloyd = MODES[mode]
        m.setOption("sa_device", device)
        params = hq.SWASA(population=P, imax=10 ** 7, seed=1).params()
        h = C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, 1, C.byref(h)), m.ctx)
        if repair:
            _lib.check(lib.hq_search_set_repair(h, repair, -1), m.ctx)
        if lloyd:
            _lib.check(lib.hq_search_set_lloyd(h, lloyd), m.ctx)
        iters = args.iters if device else max(1, args.iters // 10)  # (a host-driven iteration is a round trip)
        ran = C.c_int()

        def run():
            t0 = time.perf_counter()
            _lib.check(lib.hq_search_run(h, iters, C.byref(ran)), m.ctx)
            dt = time.perf_counter() - t0
            assert ran.value == iters
            return dt * 1e3 / iters

        for _ in range(args.warmup):
            run()
        reps = [run() for _ in range(args.reps)]
        res = {"iterations_per_call": iters, "ms_per_iteration": round(statistics.median(reps), 5),
               "ms_per_iteration_reps": [round(v, 5) for v in reps]}
        kern = {k: [] for k in KERNELS}
        lib.hq_profile_enable(m.ctx, 1)
        for _ in range(args.prof_reps):
            lib.hq_profile_reset(m.ctx)
            run()
            for k in KERNELS:
                ms, n = C.c_double(), C.c_int64()
                if lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n)) == 0 and n.value:
                    kern[k].append((ms.value / iters, n.value / iters))
        lib.hq_profile_enable(m.ctx, 0)
        res["kernel_ms_per_iteration"] = {k: round(statistics.median(v[0] for v in kern[k]), 5)
                                          for k in KERNELS if kern[k]}
        res["kernel_launches_per_iteration"] = {k: kern[k][0][1] for k in KERNELS if kern[k]}
        lib.hq_search_destroy(h)
        out[mode] = res
    m.close()
    print("RESULT " + json.dumps(out))


def run_child(args, shape, lib=None, plain_only=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--iters", str(args.iters),
           "--warmup", str(args.warmup), "--reps", str(args.reps), "--prof-reps", str(args.prof_reps)]
    if lib:
        cmd += ["--lib", os.path.abspath(lib)]
    if plain_only:
        cmd += ["--plain-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="iterations per hq_search_run call (host-driven: a tenth)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls before the timed ones (clocks settle)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--prof-reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (plain step, A/B)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_c3.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    out = {"shapes": {k: f"{v[0]}x{v[0]}, K={v[1]}, P={v[2]}" for k, v in SHAPES.items()},
           "iterations_per_call": args.iters, "warmup_calls": args.warmup, "reps": args.reps,
           "statistic": "median over reps of (host clock around hq_search_run) / iterations, profiling off; "
                        "kernel times: HIP events under hq_profile_*, separate calls, total per iteration"}
    for shape in SHAPES:
        res = run_child(args, shape)
        d, hh = res["device_repair"]["ms_per_iteration"], res["host_repair"]["ms_per_iteration"]
        kr, kp = res["device_repair"]["kernel_ms_per_iteration"], res["device_plain"]["kernel_ms_per_iteration"]
        res["repair_host_over_device"] = round(hh / d, 3)
        res["device_repair_minus_plain_ms"] = round(d - res["device_plain"]["ms_per_iteration"], 5)
        res["cost_ms"] = {"without_error_image": kp["cost"], "with_error_image": round(kr["cost"] - kp["cost"], 5)}
        res["errsum_next_to_centroid_ms"] = {"errsum": kr["errsum"],
                                             "centroid": res["device_hybrid"]["kernel_ms_per_iteration"]["centroid"]}
        if args.parent_lib:
            ab = {"parent": [], "new": []}
            for name in ("parent", "new", "new", "parent"):
                lib = args.parent_lib if name == "parent" else None
                ab[name].append(run_child(args, shape, lib, plain_only=True)["device_plain"]["ms_per_iteration_reps"])
            med = {k: statistics.median(x for run in v for x in run) for k, v in ab.items()}
            pm = {k: [statistics.median(run) for run in v] for k, v in ab.items()}
            res["plain_step_vs_parent"] = {
                "ms_per_iteration_reps": ab, "median_ms": {k: round(v, 5) for k, v in med.items()},
                "process_medians_ms": {k: [round(x, 5) for x in v] for k, v in pm.items()},
                "new_minus_parent_ms": round(med["new"] - med["parent"], 5),
                "spread_between_process_medians_ms": {k: round(abs(v[0] - v[1]), 5) for k, v in pm.items()},
                "new_over_parent": round(med["new"] / med["parent"], 4)}
        out[shape] = res
        print(shape, json.dumps(res), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
