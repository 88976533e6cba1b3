#!/usr/bin/env python3
"""Stage times of hq_kmeanspp_seed next to the other ways of preparing a start in the same process:
"kmpp_update" and "kmpp_pick" by HIP events (hq_profile_*, summed over the call's K rounds) and the
call's wall time with profiling off, against hq_set_image_planar_shard of the same image (wall time:
the call synchronises) and hq_color_histogram + hq_median_cut (the "hist" stage's HIP-event time and
the pair's wall time), at 512^2 K = 16 P = 1, 1024^2 K = 64 P = 1 and 4096^2 K = 256 P = 4.  One
process, `warmup` untimed rounds then the median of `reps` timed ones (grad_timing.py's rule).
--quality adds the best cost after 60 iterations on the 96 x 64 blob image (K = 8, population 3,
seed 17) from random, "mediancut" and "kmeans++" starts, plain and with lloydEvery = 1.
Writes profiles/kmpp_c3.json.
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
SHAPES = ((512, 16, 1), (1024, 64, 1), (4096, 256, 4))


def blob_image(np, w, h, seed):
    """A few Gaussian colour blobs rounded to bytes (the k-means tests' image)."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(40, 216, (5, 3))
    which = rng.integers(0, 5, w * h)
    by = np.clip(np.rint(centres[which] + 12.0 * rng.standard_normal((w * h, 3))), 0, 255)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    return rgba


def main():
    import numpy as np

    import hybridquantization_amd as hq
    from bench import synthetic_planes
    from hybridquantization_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmpp_c3.json"))
    args = ap.parse_args()
    lib = hq.load()
    out = {"statistic": "median over reps, ms; *_ms: HIP-event time of the stage over one call (kmpp_*: summed over "
                        "its K rounds); *_wall_ms: host clock around calls that end in a synchronise, profiling off",
           "warmup": args.warmup, "reps": args.reps, "shapes": []}

    def stage(m, name):
        ms = C.c_double()
        lib.hq_profile_get(m.ctx, name.encode(), C.byref(ms), None)
        return ms.value

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for size, K, P in SHAPES:
        m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
        sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
        R, G, B = synthetic_planes(size, size, 1)

        def set_image():
            _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), size, size,
                                                     _lib.fptr(sp.illuminant), 0, size), m.ctx)

        def median_cut():
            cells, den = m.colorHistogram(5)
            m.medianCut(cells, 5, den, K)

        keys = ("set_image_wall_ms", "hist_ms", "hist_mediancut_wall_ms", "kmpp_update_ms", "kmpp_pick_ms",
                "kmpp_seed_wall_ms")
        reps = {k: [] for k in keys}
        for r in range(args.warmup + args.reps):
            t = {"set_image_wall_ms": wall(set_image)}
            t["hist_mediancut_wall_ms"] = wall(median_cut)
            t["kmpp_seed_wall_ms"] = wall(lambda: m.kmeansppSeed(P, K, 5))
            lib.hq_profile_reset(m.ctx)
            lib.hq_profile_enable(m.ctx, 1)
            median_cut()
            m.kmeansppSeed(P, K, 5)
            lib.hq_profile_enable(m.ctx, 0)
            t.update(hist_ms=stage(m, "hist"), kmpp_update_ms=stage(m, "kmpp_update"), kmpp_pick_ms=stage(m, "kmpp_pick"))
            if r >= args.warmup:
                for k in keys:
                    reps[k].append(t[k])
        form = "packed" if m.colorHistogram(5)[1] == 255 else "planar"  # (the form hq_cluster_sums' den names)
        row = {"size": size, "K": K, "P": P, "form": form, **{k: round(statistics.median(v), 4) for k, v in reps.items()}}
        print(row, flush=True)
        out["shapes"].append(row)
        m.close()

    if args.quality:
        m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
        sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
        rgba = blob_image(np, 96, 64, 11)
        table = {}
        for init in (None, "mediancut", "kmeans++"):
            for every in (0, 1):
                sw = hq.SWASA(population=3, imax=60, seed=17)
                m.findBestQuantization(rgba.reshape(-1), None, 96, 8, sw, None, None, sp.illuminant, iterations=60,
                                       init=init, lloydEvery=every)
                table[f"{init or 'random'}{' + lloydEvery=1' if every else ''}"] = {
                    "best": m.bestError, "seed": None if init is None else m.seedError}
        print(table, flush=True)
        out["quality_blob_96x64_K8_P3_60it_seed17"] = table
        m.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
