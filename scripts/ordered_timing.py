"""What ordered dithering inside the argmin (hq_ordered_population, hq_search_set_ordered)
costs next to the plain evaluation and the plain SWASA step, and that the plain step did not
move.

    python scripts/ordered_timing.py [--parent-lib PATH] [--out profiles/ordered_c3.json]

The method is scripts/dither_timing.py's.  At C3 (4096^2, K = 256, P = 4) on the synthetic
benchmark image, per image form (the packed 8-bit copy, option "img_u8" 1, and the planar
floats, 0) one process and one context: `warmup` untimed and `reps` profiled calls of
hq_eval_population, then the same of hq_ordered_population at the heuristic amplitude
(orderedAmplitude(K)) under the default map and under a 64 x 64 Bayer map, with the same P
random palettes.  The times are HIP events carried by the launches (hq_profile_*), medians
over the reps with every rep beside them.

Then the search step in a process of its own: a device-resident plain search and one under
the ordered cost, `step-warmup` untimed hq_search_run calls of `step-iters` iterations and
`step-reps` timed ones each (a host clock around the call, which ends in a stream
synchronise), profiling off.

Then one observation, no gate: on the 128 x 128 benchmark image (K = 8, P = 3, seed 17, 60
iterations) the ordered cost of the plain search's best palette against the best of a
search under the ordered cost.

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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import repair_timing  # noqa: E402

SIZE, K, P = 4096, 256, 4  # C3
KERNELS = ("grid", "assign", "cost", "finalize")


def _context(img_u8):
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.setOption("img_u8", img_u8)
    R, G, B = synthetic_planes(SIZE, SIZE, 1)
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), SIZE, SIZE,
                                             _lib.fptr(sp.illuminant), 0, SIZE), m.ctx)
    return hq, _lib, lib, m


def child_eval(args):
    import numpy as np

    hq, _lib, lib, m = _context(args.img_u8)
    amp = hq.ImageManipulation.orderedAmplitude(K)
    pals = np.random.default_rng(K).random((P, 4 * K), np.float32)
    pals[:, 3::4] = 0.0
    out = {"img_u8": args.img_u8, "amp": amp}
    lib.hq_profile_enable(m.ctx, 1)

    def ordered_with(tmap):
        def call():
            m.setDitherMap(tmap)
            return m.orderedPopulation(pals, amp, 2.0)
        return call

    calls = {"plain": lambda: m.computeQuantizationErrorPopulation(pals, 2.0),
             "ordered_bayer16": ordered_with(None),
             "ordered_bayer64": ordered_with(hq.ImageManipulation.bayerMap(6)),
             "plain_again": lambda: m.computeQuantizationErrorPopulation(pals, 2.0)}
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
    a = {k: out[k]["kernel_ms_per_launch"]["assign"] for k in calls}
    out["assign_ms"] = a
    out["ordered_over_plain_assign"] = {k: round(a[k] / a["plain"], 4) for k in ("ordered_bayer16", "ordered_bayer64")}
    print("RESULT " + json.dumps(out))


def child_step(args):
    import numpy as np

    hq, _lib, lib, m = _context(1)
    amp = np.full(3, hq.ImageManipulation.orderedAmplitude(K), np.float32)
    out = {"amp": float(amp[0]), "iterations_per_call": args.step_iters}
    for mode in ("plain", "ordered"):
        params = hq.SWASA(population=P, imax=10 ** 7, seed=1).params()
        h = C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, 1, C.byref(h)), m.ctx)
        if mode == "ordered":
            _lib.check(lib.hq_search_set_ordered(h, _lib.fptr(amp)), m.ctx)
        ran = C.c_int()

        def run():
            t0 = time.perf_counter()
            _lib.check(lib.hq_search_run(h, args.step_iters, C.byref(ran)), m.ctx)
            dt = time.perf_counter() - t0
            assert ran.value == args.step_iters
            return dt * 1e3 / args.step_iters

        for _ in range(args.step_warmup):
            run()
        reps = [run() for _ in range(args.step_reps)]
        out[mode] = {"ms_per_iteration": round(statistics.median(reps), 5),
                     "ms_per_iteration_reps": [round(v, 5) for v in reps]}
        lib.hq_search_destroy(h)
    m.close()
    out["ordered_minus_plain_ms"] = round(out["ordered"]["ms_per_iteration"] - out["plain"]["ms_per_iteration"], 5)
    print("RESULT " + json.dumps(out))


def search_observation():
    import numpy as np
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd.scielab_processor import makeinline

    w, k, p, iters = 128, 8, 3, 60
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    rgba = makeinline(np.stack(synthetic_planes(w, w, 1)))
    out = {"image": f"{w}x{w} benchmark image", "K": k, "P": p, "iterations": iters, "seed": 17, "dE": "CIE76"}
    for amp in (hq.ImageManipulation.orderedAmplitude(k), 0.5, 0.2):
        res = {}
        for name, kw in (("plain_search_then_ordered", dict(ordered=amp)),
                         ("ordered_search", dict(ordered=amp, orderedSearch=True))):
            sw = hq.SWASA(population=p, imax=iters, seed=17)
            m.findBestQuantization(rgba, None, w, k, sw, None, None, sp.illuminant, iterations=iters, **kw)
            res[name] = {"bestError": m.bestError, "bestErrorOrdered": m.bestErrorOrdered}
        out[f"amp_{amp:g}"] = res
    m.close()
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
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls before the profiled ones")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (plain C3 step, A/B)")
    ap.add_argument("--step-iters", type=int, default=200, help="iterations per hq_search_run call")
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--step-reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ordered_c3.json"))
    ap.add_argument("--child", default=None, choices=("eval", "step", "observe"), help=argparse.SUPPRESS)
    ap.add_argument("--img-u8", type=int, default=1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "eval":
        return child_eval(args)
    if args.child == "step":
        return child_step(args)
    if args.child == "observe":
        return search_observation()
    out = {"shape": f"C3: {SIZE}x{SIZE}, K={K}, P={P}, dE76, 72 dpi / 45 cm",
           "warmup_calls": args.warmup, "reps": args.reps,
           "statistic": "median over reps of the HIP-event time of each kernel's launch under hq_profile_*; the "
                        "search step: median over reps of the host time of hq_search_run / iterations",
           "not_measured": "more than one GPU (the collective is the plain evaluation's; no run on N > 1), and "
                           "K > 256 (refused: HQ_ERR_UNSUPPORTED)",
           "for_comparison": "the Floyd-Steinberg kernel takes 336.7 ms per palette at this shape "
                             "(profiles/dither_c3.json)"}
    for img_u8 in (1, 0):
        key = "packed_u8" if img_u8 else "planar_f32"
        out[key] = run_self(args, "--child", "eval", "--img-u8", str(img_u8))
        print(key, json.dumps(out[key]["assign_ms"]), flush=True)
    out["search_step"] = run_self(args, "--child", "step")
    print(json.dumps(out["search_step"]), flush=True)
    out["ordered_search_observation"] = run_self(args, "--child", "observe")
    print(json.dumps(out["ordered_search_observation"]), flush=True)
    if args.parent_lib:
        step = argparse.Namespace(iters=args.step_iters, warmup=args.step_warmup, reps=args.step_reps, prof_reps=1,
                                  timeout=args.timeout)
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
