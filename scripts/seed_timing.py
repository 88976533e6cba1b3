"""What seeding a search from the image costs on the device: the `hist` kernel of
hq_color_histogram at 4096^2 and bits = 5, timed by hq_profile_* next to the
once-per-image work it joins (hq_set_image of the same image, a host clock) and
next to `centroid` (hq_cluster_sums, P = 1, K = 256) on the same image, in the
same process.

    python scripts/seed_timing.py [--parent-lib PATH] [--out profiles/seed_c3.json]

Three images, a fresh process each (one library and one context per process):
  noise      the synthetic benchmark image (uniform bytes: almost every pixel a cell of its own)
  clustered  16 Gaussian colour blobs rounded to bytes (a few cells take most pixels)
  single     one colour: every pixel in one cell, the worst case of same-address atomics
Per image and form (packed bytes, and the planar floats with option img_u8 0):
`warmup` rounds of (hq_color_histogram, hq_eval_population, hq_cluster_sums),
then `reps` timed rounds under hq_profile_* (HIP events carried by the launches);
hq_set_image_planar_shard is timed `reps` times by a host clock after one untimed
call.  Medians are reported with every repetition beside them.

--parent-lib: a libhq.so built from the parent commit.  The plain
device-resident search step (no seed, every = 0) at C3 (4096^2, K = 256, P = 4)
and C2 (1024^2, K = 64, P = 1) is timed on it and on this tree's in processes of
their own, alternating (parent, new, new, parent), so the difference can be read
against the spread between process medians of one library.
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

IMAGES = ("noise", "clustered", "single")
KERNELS = ("hist", "centroid", "assign")
SHAPES = {"C3": (4096, 256, 4), "C2": (1024, 64, 1)}


def child_image(args):
    import numpy as np

    from lloyd_timing import planes

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    W = H = args.size
    K, bits = args.K, args.bits
    R, G, B = planes(args.child, W, H)

    def set_image():
        t0 = time.perf_counter()
        _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), W, H,
                                                 _lib.fptr(sp.illuminant), 0, H), m.ctx)
        return (time.perf_counter() - t0) * 1e3

    set_image()
    set_ms = [set_image() for _ in range(args.reps)]
    pal = np.zeros((1, K, 4), np.float32)
    pal[..., :3] = np.random.default_rng(2).random((1, K, 3), np.float32)
    pal = np.ascontiguousarray(pal.reshape(1, -1))
    costs = np.zeros(1, np.float64)
    sums = np.zeros((1, K, 4), np.int64)
    cells = np.zeros((1 << (3 * bits), 4), np.int64)
    den, hden = C.c_int64(), C.c_int64()

    def one_round():
        _lib.check(lib.hq_color_histogram(m.ctx, bits, _lib.i64ptr(cells), C.byref(hden)), m.ctx)
        _lib.check(lib.hq_eval_population(m.ctx, _lib.fptr(pal), 1, K, 2.0, _lib.dptr(costs), None), m.ctx)
        _lib.check(lib.hq_cluster_sums(m.ctx, 1, K, _lib.i64ptr(sums), C.byref(den)), m.ctx)

    out = {"image": args.child, "set_image_ms": round(statistics.median(set_ms), 3),
           "set_image_ms_reps": [round(v, 3) for v in set_ms]}
    for form, u8 in (("packed", 1), ("planar", 0)):
        m.setOption("img_u8", u8)
        for _ in range(args.warmup):
            one_round()
        reps = {k: [] for k in KERNELS}
        for _ in range(args.reps):
            lib.hq_profile_reset(m.ctx)
            lib.hq_profile_enable(m.ctx, 1)
            one_round()
            lib.hq_profile_enable(m.ctx, 0)
            for k in KERNELS:
                ms, n = C.c_double(), C.c_int64()
                _lib.check(lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n)), m.ctx)
                reps[k].append(ms.value / max(n.value, 1))
        assert hden.value == den.value == (255 if u8 else 1 << 32), (hden.value, den.value)  # (every image here is k/255)
        assert int(cells[:, 3].sum()) == W * H == int(sums[..., 3].sum())
        assert np.array_equal(cells[:, :3].sum(0), sums[0, :, :3].sum(0))  # the same pixels, parted differently
        out[form] = {"den": hden.value, "cells_with_pixels": int(np.count_nonzero(cells[:, 3])),
                     **{f"{k}_ms": round(statistics.median(reps[k]), 4) for k in KERNELS},
                     **{f"{k}_ms_reps": [round(v, 4) for v in reps[k]] for k in KERNELS}}
        out[form]["hist_over_set_image"] = round(out[form]["hist_ms"] / out["set_image_ms"], 5)
    m.close()
    print("RESULT " + json.dumps(out))


def child_search(args):
    from bench import synthetic_planes
    from hybrid_timing import load_lib

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = load_lib(args.lib) if args.lib else hq.load()
    size, K, P = SHAPES[args.child]
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    R, G, B = synthetic_planes(size, size, 1)
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), size, size,
                                             _lib.fptr(sp.illuminant), 0, size), m.ctx)
    params = hq.SWASA(population=P, imax=10 ** 7, seed=1).params()
    h = C.c_void_p()
    _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, 1, C.byref(h)), m.ctx)
    ran = C.c_int()

    def run():
        t0 = time.perf_counter()
        _lib.check(lib.hq_search_run(h, args.iters, C.byref(ran)), m.ctx)
        dt = time.perf_counter() - t0
        assert ran.value == args.iters
        return dt * 1e3 / args.iters

    for _ in range(args.search_warmup):
        run()
    reps = [run() for _ in range(args.reps)]
    lib.hq_search_destroy(h)
    m.close()
    print("RESULT " + json.dumps({"shape": args.child, "lib": args.lib or "this tree",
                                  "ms_per_iteration_reps": [round(v, 5) for v in reps]}))


def run_child(args, kind, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--size", str(args.size), "--K", str(args.K),
           "--bits", str(args.bits), "--warmup", str(args.warmup), "--reps", str(args.reps), "--iters", str(args.iters),
           "--search-warmup", str(args.search_warmup)]
    if lib:
        cmd += ["--lib", os.path.abspath(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--K", type=int, default=256, help="colours of the palette behind the centroid comparison")
    ap.add_argument("--bits", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10, help="untimed rounds before the timed ones (clocks settle)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200, help="plain search: iterations per hq_search_run call")
    ap.add_argument("--search-warmup", type=int, default=3, help="plain search: untimed calls before the timed ones")
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (plain search step, A/B)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_c3.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child in IMAGES:
        return child_image(args)
    if args.child in SHAPES:
        return child_search(args)
    n = args.size * args.size
    out = {"shape": f"{args.size}x{args.size}, bits={args.bits}; centroid: P=1, K={args.K}",
           "warmup_rounds": args.warmup, "reps": args.reps,
           "statistic": "median over reps; hist, centroid, assign: the HIP-event time per launch, one round = "
                        "hq_color_histogram + hq_eval_population + hq_cluster_sums; set_image: a host clock "
                        "around hq_set_image_planar_shard (upload, packing, S-CIELAB of the image)",
           "atomic_bytes_if_every_pixel_its_own_cell": n * 32}
    for kind in IMAGES:
        out[kind] = run_child(args, kind)
        print(kind, json.dumps(out[kind]), flush=True)
    if args.parent_lib:
        out["plain_step_vs_parent"] = {"shapes": {k: f"{v[0]}x{v[0]}, K={v[1]}, P={v[2]}" for k, v in SHAPES.items()},
                                       "iterations_per_call": args.iters, "warmup_calls": args.search_warmup}
        for shape in SHAPES:
            ab = {"parent": [], "new": []}
            for name in ("parent", "new", "new", "parent"):
                ab[name].append(run_child(args, shape, args.parent_lib if name == "parent" else None)
                                ["ms_per_iteration_reps"])
            med = {k: statistics.median(x for run in v for x in run) for k, v in ab.items()}
            pm = {k: [round(statistics.median(run), 5) for run in v] for k, v in ab.items()}
            out["plain_step_vs_parent"][shape] = {
                "ms_per_iteration_reps": ab, "process_median_ms": pm,
                "median_ms": {k: round(v, 5) for k, v in med.items()},
                "new_over_parent": round(med["new"] / med["parent"], 4)}
            print(shape, json.dumps(out["plain_step_vs_parent"][shape]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
