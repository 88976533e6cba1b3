"""What CIEDE2000 costs on the device: the C3 shape (4096^2, K = 256, P = 4) timed
for CIE76 and CIEDE2000 contexts in the same run on the same GPU, through the
Python mirror and hq_profile_*.

    python scripts/de2000_timing.py [--parent-lib PATH] [--out profiles/de2000_c3.json]

Per dE type, in a fresh process each (one library and one context per process):
`warmup` device-resident SA steps, then `reps` timed regions of `steps` steps
(wall time per step: the whole SA step) and `reps` regions under hq_profile_*
(the `cost` kernel's HIP-event time per launch).  Medians are reported, with
every repetition beside them.  --parent-lib: a libhq.so built from the parent
commit, timed the same way with CIE76, so that "no dE76 kernel changed" can be
read off this GPU's own run-to-run spread.
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

NAMES = {0: "CIE76", 2: "CIEDE2000"}


def child(args):
    import numpy as np

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib
    from bench import synthetic_planes

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    lib = hq.load()
    m = hq.ImageManipulation(args.child, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    W = H = args.size
    R, G, B = synthetic_planes(W, H, 1)
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), W, H,
                                             _lib.fptr(sp.illuminant), 0, H), m.ctx)
    sw = hq.SWASA(population=args.P, imax=10 ** 9, seed=1)
    params = sw.params()
    s = C.c_void_p()
    _lib.check(lib.hq_search_create(m.ctx, C.byref(params), args.K, sw.seed, C.byref(s)), m.ctx)
    ran = C.c_int()
    _lib.check(lib.hq_search_run(s, args.warmup, C.byref(ran)), m.ctx)
    step_ms, cost_ms = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        _lib.check(lib.hq_search_run(s, args.steps, C.byref(ran)), m.ctx)  # (returns after the stream has drained)
        step_ms.append((time.perf_counter() - t0) / args.steps * 1e3)
    for _ in range(args.reps):
        lib.hq_profile_reset(m.ctx)
        lib.hq_profile_enable(m.ctx, 1)
        _lib.check(lib.hq_search_run(s, args.steps, C.byref(ran)), m.ctx)
        lib.hq_profile_enable(m.ctx, 0)
        ms, n = C.c_double(), C.c_int64()
        lib.hq_profile_get(m.ctx, b"cost", C.byref(ms), C.byref(n))
        cost_ms.append(ms.value / max(n.value, 1))
    best = np.zeros(4 * args.K, np.float32)
    err, it = C.c_double(), C.c_int()
    lib.hq_search_best(s, _lib.fptr(best), C.byref(err), C.byref(it))
    lib.hq_search_destroy(s)
    m.close()
    print("RESULT " + json.dumps({
        "delta_e": NAMES[args.child], "lib": os.path.basename(args.lib or "libhq.so"),
        "step_ms": round(statistics.median(step_ms), 4), "cost_kernel_ms": round(statistics.median(cost_ms), 4),
        "step_ms_reps": [round(v, 4) for v in step_ms], "cost_kernel_ms_reps": [round(v, 4) for v in cost_ms],
        "best_error": err.value, "iterations": it.value}))


def run_child(args, de, libpath):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(de), "--size", str(args.size), "--K", str(args.K),
           "--P", str(args.P), "--steps", str(args.steps), "--warmup", str(args.warmup), "--reps", str(args.reps)]
    if libpath:
        cmd += ["--lib", libpath]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--P", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=300, help="SA steps before the first timed region (clocks settle)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (CIE76 only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "de2000_c3.json"))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    # the two CIE76 runs bracket the CIEDE2000 one; the parent's comes between them again
    runs = [("cie76", 0, None), ("ciede2000", 2, None)]
    if args.parent_lib:
        runs.append(("parent_cie76", 0, args.parent_lib))
    runs.append(("cie76_again", 0, None))
    out = {"shape": f"{args.size}x{args.size}, K={args.K}, P={args.P} (BASELINE config 3 at the defaults), "
                    "device-resident SWASA steps",
           "steps_per_region": args.steps, "warmup_steps": args.warmup, "reps": args.reps,
           "statistic": "median over reps; step_ms = wall time per SA step, cost_kernel_ms = HIP events"}
    for name, de, libpath in runs:
        out[name] = run_child(args, de, libpath)
        print(name, json.dumps(out[name]), flush=True)
    a, b = out["cie76"], out["ciede2000"]
    out["ciede2000_over_cie76"] = {"step": round(b["step_ms"] / a["step_ms"], 3),
                                   "cost_kernel": round(b["cost_kernel_ms"] / a["cost_kernel_ms"], 3)}
    spread = [v for k in ("cie76", "cie76_again") for v in out[k]["step_ms_reps"]]
    out["cie76_step_ms_spread"] = [min(spread), max(spread)]
    if args.parent_lib:
        out["cie76_over_parent_cie76_step"] = round(a["step_ms"] / out["parent_cie76"]["step_ms"], 4)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in out if k.startswith(("ciede2000_over", "cie76_over", "cie76_step"))}))


if __name__ == "__main__":
    main()
