#!/usr/bin/env python3
"""The descent move inside the search (hq_search_set_descend), measured in one process:

  stages   per-iteration HIP-event times (hq_profile_*) of a device-resident search with
           descendEvery = 1 -- "descend", the assign-only pass ("grid" + "assign" above the plain
           step's), "grad_pixel", "grad_adjoint" -- next to the plain step's own stages, at 512^2
           K = 16, 1024^2 K = 64 and the C3 shape (4096^2, K = 256, P = 4);
  wall     the wall time per iteration of the plain search, of the device-resident search with a
           descent move in every iteration and of the host-driven one (option sa_device 0);
  quality  blob image, K = 8, population 3, seed 17, 60 iterations: the best cost of the plain
           search, lloydEvery = 1, descendEvery 1 and 5, both moves together and the median-cut start,
           each with and without descendSteps = 8.

`warmup` untimed runs then the median of `reps` timed ones.  Writes profiles/descend_search_c3.json.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("sa_step", "grid", "assign", "cost", "grad_pixel", "grad_adjoint", "descend")
SHAPES = ((512, 16, 1), (1024, 64, 1), (4096, 256, 4))
RATE = 1e-3


def run(lib, _lib, hq, m, K, P, iters, every, device, profile):
    """One search of `iters` iterations -> (wall ms per iteration, stage ms per iteration)."""
    m.setOption("sa_device", device)
    params = hq.SWASA(population=P, imax=iters, seed=17).params()
    h = C.c_void_p()
    _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, 17, C.byref(h)), m.ctx)
    try:
        _lib.check(lib.hq_search_set_descend(h, every, RATE), m.ctx)
        lib.hq_profile_reset(m.ctx)
        lib.hq_profile_enable(m.ctx, 1 if profile else 0)
        t0 = time.perf_counter()
        _lib.check(lib.hq_search_run(h, iters, None), m.ctx)
        wall = (time.perf_counter() - t0) * 1e3 / iters
        lib.hq_profile_enable(m.ctx, 0)
        stages = {}
        for k in STAGES:
            ms = C.c_double()
            lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), None)
            stages[k] = ms.value / iters
        return wall, stages
    finally:
        lib.hq_search_destroy(h)


def median_of(fn, warmup, reps):
    rows = [fn() for _ in range(warmup + reps)][warmup:]
    wall = statistics.median(r[0] for r in rows)
    return round(wall, 4), {k: round(statistics.median(r[1][k] for r in rows), 4) for k in STAGES}


def quality(hq, np):
    w, h, K = 96, 64, 8
    rng = np.random.default_rng(11)  # tests/test_lloyd_gpu.py's blob_image(96, 64, seed=11)
    centres = rng.integers(40, 216, (5, 3))
    which = rng.integers(0, 5, w * h)
    by = np.clip(np.rint(centres[which] + 12.0 * rng.standard_normal((w * h, 3))), 0, 255)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    rows = {}
    for name, kw in (("plain", {}), ("lloydEvery=1", dict(lloydEvery=1)), ("descendEvery=1", dict(descendEvery=1)),
                     ("descendEvery=5", dict(descendEvery=5)),
                     ("descendEvery=1 lloydEvery=1", dict(descendEvery=1, lloydEvery=1)),
                     ("descendEvery=5 lloydEvery=1", dict(descendEvery=5, lloydEvery=1)),
                     ("init=mediancut", dict(init="mediancut")),
                     ("init=mediancut descendEvery=1", dict(init="mediancut", descendEvery=1))):
        for steps in (0, 8):
            sw = hq.SWASA(population=3, imax=60, seed=17)
            m.findBestQuantization(rgba.reshape(-1), None, w, K, sw, None, None, sp.illuminant, iterations=60,
                                   descendSteps=steps, **kw)
            rows[name + (" + descendSteps=8" if steps else "")] = round(float(m.bestError), 5)
            print(name, steps, m.bestError, flush=True)
    m.close()
    return {"image": "blob_image(96, 64, seed=11)", "settings": "K=8, population 3, seed 17, 60 iterations, "
            "descendRate 1e-3", "best_cost": rows}


def main():
    import numpy as np

    import hybridquantization_amd as hq
    from bench import synthetic_planes
    from hybridquantization_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "descend_search_c3.json"))
    args = ap.parse_args()
    lib = hq.load()
    out = {"statistic": "median over reps of one search run of `iters` iterations, per iteration, ms: HIP-event stage "
                        "times (profiling on) and wall times (profiling off)",
           "warmup": args.warmup, "reps": args.reps, "iters": args.iters, "rate": RATE, "shapes": []}
    for size, K, P in SHAPES:
        m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
        sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
        R, G, B = synthetic_planes(size, size, 1)
        _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), size, size,
                                                 _lib.fptr(sp.illuminant), 0, size), m.ctx)
        go = lambda every, device, prof: median_of(  # noqa: E731
            lambda: run(lib, _lib, hq, m, K, P, args.iters, every, device, prof), args.warmup, args.reps)
        row = {"size": size, "K": K, "P": P, "half": m.halfSize}
        _, row["plain_stages_ms"] = go(0, 1, True)
        _, row["descend_stages_ms"] = go(1, 1, True)
        row["wall_ms"] = {"plain_device": go(0, 1, False)[0], "descend_device": go(1, 1, False)[0],
                          "descend_host_driven": go(1, 0, False)[0], "plain_host_driven": go(0, 0, False)[0]}
        print(json.dumps(row), flush=True)
        out["shapes"].append(row)
        m.close()
    out["quality"] = quality(hq, np)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
