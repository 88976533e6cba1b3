#!/usr/bin/env python3
"""Stage times of hq_cost_gradient next to the cost and the k-means sums of the same process:
grad_pixel and grad_adjoint of the tiled form and of the plain pair (option "grad_tiled"), against
"cost" and "centroid", by HIP events (hq_profile_*), at 512^2 K = 16, 1024^2 K = 64 and the C3 shape
(4096^2, K = 256, P = 4).  One process, `warmup` untimed rounds then the median of `reps` timed
ones; a round = hq_eval_population, hq_cluster_sums, hq_cost_gradient.  Writes profiles/grad_c3.json.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("cost", "centroid", "grad_pixel", "grad_adjoint")
SHAPES = ((512, 16, 1), (1024, 64, 1), (4096, 256, 4))


def main():
    import numpy as np

    import hybridquantization_amd as hq
    from bench import synthetic_planes
    from hybridquantization_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_c3.json"))
    args = ap.parse_args()
    lib = hq.load()
    out = {"statistic": "median over reps of the HIP-event time per stage and call, ms; a round = hq_eval_population, "
                        "hq_cluster_sums, hq_cost_gradient", "warmup": args.warmup, "reps": args.reps, "shapes": []}
    for size, K, P in SHAPES:
        m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
        sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
        R, G, B = synthetic_planes(size, size, 1)
        _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), size, size,
                                                 _lib.fptr(sp.illuminant), 0, size), m.ctx)
        pals = np.zeros((P, K, 4), np.float32)
        pals[..., :3] = np.random.default_rng(2).random((P, K, 3), np.float32)
        pals = np.ascontiguousarray(pals.reshape(P, -1))
        costs, sums, den = np.zeros(P), np.zeros((P, K, 4), np.int64), C.c_int64()
        grad = np.zeros((P, K, 4))
        row = {"size": size, "K": K, "P": P, "half": m.halfSize}
        for form, name in ((1, "tiled"), (0, "plain")):
            m.setOption("grad_tiled", form)
            reps = {k: [] for k in STAGES}
            for r in range(args.warmup + args.reps):
                lib.hq_profile_reset(m.ctx)
                lib.hq_profile_enable(m.ctx, 1)
                _lib.check(lib.hq_eval_population(m.ctx, _lib.fptr(pals), P, K, 2.0, _lib.dptr(costs), None), m.ctx)
                _lib.check(lib.hq_cluster_sums(m.ctx, P, K, _lib.i64ptr(sums), C.byref(den)), m.ctx)
                _lib.check(lib.hq_cost_gradient(m.ctx, P, K, _lib.dptr(grad)), m.ctx)
                lib.hq_profile_enable(m.ctx, 0)
                for k in STAGES:
                    ms, n = C.c_double(), C.c_int64()
                    lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n))
                    if r >= args.warmup:
                        reps[k].append(ms.value)
            row[name] = {f"{k}_ms": round(statistics.median(reps[k]), 4) for k in STAGES}
            print(size, K, P, name, row[name], flush=True)
        out["shapes"].append(row)
        m.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
