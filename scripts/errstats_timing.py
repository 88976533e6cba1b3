#!/usr/bin/env python3
"""Stage time of hq_error_stats ("errstats", HIP events through hq_profile_*, per call) at nbins = 256,
top = 50 next to the same run's "errsum" stage (hq_cluster_errors on the same evaluation) and a
device-to-device copy of the P error planes' bytes (torch, CUDA events: the read floor), at 512^2
K = 16 P = 1, 1024^2 K = 64 P = 1 and 4096^2 K = 256 P = 4.  Then the stage alone, call after call, on
the largest shape: on the noise image's error image and on a flat image's, whose pixels all land in
one bin (the LDS atomics' worst case).  `warmup` untimed rounds, then the median and the range of
`reps` timed ones (grad_timing.py's rule).  Writes profiles/errstats_c3.json.
(profiles/errstats_lds_forms.json: this script's output when the kernel still had a second LDS form,
a histogram per wave under an option "errstats_waves" -- the measurement that removed it.)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((512, 16, 1), (1024, 64, 1), (4096, 256, 4))
NBINS, TOP = 256, 50.0


def main():
    import numpy as np
    import torch

    import hybridquantization_amd as hq
    from bench import synthetic_planes
    from hybridquantization_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "errstats_c3.json"))
    args = ap.parse_args()
    lib = hq.load()
    out = {"statistic": "[median, min, max] over reps, ms per call; errstats, errsum: HIP-event time of the stage; "
                        "copy: device-to-device copy of P planes of 4 W H bytes",
           "nbins": NBINS, "top": TOP, "warmup": args.warmup, "reps": args.reps, "shapes": [], "concentration": []}

    def staged(m, name, call):
        """The stage's time per launch over one profiled call."""
        ms, n = C.c_double(), C.c_int64()
        lib.hq_profile_reset(m.ctx)
        lib.hq_profile_enable(m.ctx, 1)
        call()
        lib.hq_profile_enable(m.ctx, 0)
        lib.hq_profile_get(m.ctx, name.encode(), C.byref(ms), C.byref(n))
        return ms.value / n.value

    def summary(v):
        return [round(statistics.median(v), 5), round(min(v), 5), round(max(v), 5)]

    def evaluated(size, K, P, planes):
        m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
        sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
        m.setOption("pixel_err", 1)
        _lib.check(lib.hq_set_image_planar_shard(m.ctx, *(_lib.fptr(c) for c in planes), size, size,
                                                 _lib.fptr(sp.illuminant), 0, size), m.ctx)
        m.w = m.h = size
        pals = np.zeros((P, K, 4), np.float32)
        pals[..., :3] = np.random.default_rng(7).random((P, K, 3))
        m.computeQuantizationErrorPopulation(pals.reshape(P, -1), 2.0)
        return m

    for size, K, P in SHAPES:
        m = evaluated(size, K, P, synthetic_planes(size, size, 1))
        src = torch.zeros(P * size * size, dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
        t = {"errstats": [], "errsum": [], "copy": []}
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            one = {"errstats": staged(m, "errstats", lambda: m.errorStats(P, NBINS, TOP)),
                   "errsum": staged(m, "errsum", lambda: m.clusterErrors(P, K)), "copy": e0.elapsed_time(e1)}
            if r >= args.warmup:
                for k, v in one.items():
                    t[k].append(v)
        hist = m.errorStats(P, NBINS, TOP)[0]
        row = {"size": size, "K": K, "P": P, **{k: summary(v) for k, v in t.items()},
               "errstats_over_copy": round(statistics.median(t["errstats"]) / statistics.median(t["copy"]), 3),
               "largest_bin_share": round(float(hist.max(axis=1).sum() / hist.sum()), 4)}
        print(row, flush=True)
        out["shapes"].append(row)
        m.close()

    size, K, P = SHAPES[-1]
    flat = tuple(np.full(size * size, v, np.float32) for v in (0.25, 0.5, 0.75))
    for name, planes in (("noise", synthetic_planes(size, size, 1)), ("flat", flat)):
        m = evaluated(size, K, P, planes)
        t = [staged(m, "errstats", lambda: m.errorStats(P, NBINS, TOP)) for r in range(args.warmup + args.reps)]
        hist = m.errorStats(P, NBINS, TOP)[0]
        row = {"image": name, "size": size, "K": K, "P": P, "errstats": summary(t[args.warmup:]),
               "largest_bin_share": round(float(hist.max(axis=1).sum() / hist.sum()), 4)}
        print(row, flush=True)
        out["concentration"].append(row)
        m.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
