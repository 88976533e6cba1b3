"""What the per-colour sums cost on the device: the `centroid` kernel of
hq_cluster_sums at the C3 shape (4096^2, K = 256, P = 4), timed by hq_profile_*
next to `assign` and `cost` of the evaluation it follows, in the same process.

    python scripts/lloyd_timing.py [--hbm-gbs RATE] [--out profiles/lloyd_c3.json]

Three images, a fresh process each (one library and one context per process):
  noise      the synthetic benchmark image (uniform bytes: every colour in use)
  clustered  16 Gaussian colour blobs rounded to bytes (a few colours take most pixels)
  single     one colour: every pixel on one accumulator, the worst case of
             same-address LDS atomics
Per image and form (packed bytes, and the planar floats with option img_u8 0):
`warmup` rounds of (hq_eval_population, hq_cluster_sums), then `reps` timed
rounds under hq_profile_* (HIP events carried by the launches).  Medians are
reported with every repetition beside them.  The read-traffic floor is counted
bytes -- the pixels once per population (4 B packed, 12 B planar) plus one index
byte per pixel and palette -- over --hbm-gbs, the HBM rate the same machine
reaches in its own `bench.py --full` run (roofline.hbm_GBs_alg), not the data
sheet's; without the option the floor is left out.
"""

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGES = ("noise", "clustered", "single")
KERNELS = ("centroid", "assign", "cost")


def planes(kind, W, H):
    import numpy as np

    from bench import synthetic_planes

    if kind == "noise":
        return synthetic_planes(W, H, 1)
    if kind == "single":
        return [np.full(W * H, np.float32(k) / np.float32(255), np.float32) for k in (128, 64, 200)]
    rng = np.random.default_rng(1)
    centres = rng.integers(30, 226, (16, 3))
    which = rng.integers(0, 16, W * H)
    by = np.clip(np.rint(centres[which] + 10.0 * rng.standard_normal((W * H, 3))), 0, 255).astype(np.int64)
    return [np.ascontiguousarray(by[:, c].astype(np.float32) / np.float32(255)) for c in range(3)]


def child(args):
    import numpy as np

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    W = H = args.size
    P, K = args.P, args.K
    R, G, B = planes(args.child, W, H)
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), W, H,
                                             _lib.fptr(sp.illuminant), 0, H), m.ctx)
    pals = np.zeros((P, K, 4), np.float32)  # uniform random colours, .w = 0
    pals[..., :3] = np.random.default_rng(2).random((P, K, 3), np.float32)
    pals = np.ascontiguousarray(pals.reshape(P, -1))
    costs = np.zeros(P, np.float64)
    sums = np.zeros((P, K, 4), np.int64)
    den = C.c_int64()

    def one_round():
        _lib.check(lib.hq_eval_population(m.ctx, _lib.fptr(pals), P, K, 2.0, _lib.dptr(costs), None), m.ctx)
        _lib.check(lib.hq_cluster_sums(m.ctx, P, K, _lib.i64ptr(sums), C.byref(den)), m.ctx)

    out = {"image": args.child}
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
                lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n))
                reps[k].append(ms.value / max(n.value, 1))
        assert den.value == (255 if u8 else 1 << 32), den.value  # (every image here is k/255)
        colours_used = int((sums[..., 3] > 0).sum())
        assert int(sums[..., 3].sum()) == P * W * H
        out[form] = {"den": den.value, "colours_with_pixels": colours_used,
                     **{f"{k}_ms": round(statistics.median(reps[k]), 4) for k in KERNELS},
                     **{f"{k}_ms_reps": [round(v, 4) for v in reps[k]] for k in KERNELS}}
    m.close()
    print("RESULT " + json.dumps(out))


def run_child(args, kind):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--size", str(args.size), "--K", str(args.K),
           "--P", str(args.P), "--warmup", str(args.warmup), "--reps", str(args.reps)]
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
    ap.add_argument("--warmup", type=int, default=20, help="untimed rounds before the timed ones (clocks settle)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--hbm-gbs", type=float, default=None,
                    help="HBM rate of this machine's own bench.py --full run (roofline.hbm_GBs_alg), GB/s")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lloyd_c3.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    n = args.size * args.size
    out = {"shape": f"{args.size}x{args.size}, K={args.K}, P={args.P} (BASELINE config 3 at the defaults)",
           "warmup_rounds": args.warmup, "reps": args.reps,
           "statistic": "median over reps of the HIP-event time per launch; one round = hq_eval_population + "
                        "hq_cluster_sums",
           "read_bytes": {"packed": n * (4 + args.P), "planar": n * (12 + args.P)},
           "hbm_gbs_of_bench_run": args.hbm_gbs}
    for kind in IMAGES:
        res = run_child(args, kind)
        for form in ("packed", "planar"):
            f = res[form]
            f["centroid_over_assign"] = round(f["centroid_ms"] / f["assign_ms"], 3)
            if args.hbm_gbs:
                f["read_floor_ms"] = round(out["read_bytes"][form] / (args.hbm_gbs * 1e9) * 1e3, 4)
        out[kind] = res
        print(kind, json.dumps(res), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
