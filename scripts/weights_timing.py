"""What pixel weights (hq_set_weights) cost at C3, that the plain and masked paths did not move,
what the tile skip buys under weights, and one quality example.

    python scripts/weights_timing.py [--parent-lib PATH] [--out profiles/weights_c3.json]

The method is scripts/mask_timing.py's, whose code this runs.  C3 (4096^2, K = 256, P = 4, dE76)
on the synthetic benchmark image; HIP-event stages, a host clock around hq_search_run, medians of
`reps` after `warmup` untimed rounds.

price: one process, one context, bracketed: nothing set, an all-ones mask, all-255 weights (both
with option "mask_skip" 0: every tile launched), nothing set again -- the `cost`, `centroid` and
`hist` stages per launch and the device-resident search step.  Then the same four on the planar
image form (option "img_u8" 0), whose `centroid` layout is another; its weights are all 127,
because all 255 on 4096^2 sum to 2^32 >= 2^31 and the planar sums refuse that.

skip: one process, a centred square of 1/4 of the area as weights (255 inside, 0 outside),
"mask_skip" 1 against 0.

quality: the test blob image (96 x 64, 5 Gaussian blobs), one blob weighted 255 and the rest 1,
K = 8, population 3, seed 17, lloydEvery = 1, 60 iterations: the weighted cost of the weighted
search's palette against that of the unweighted search's palette under the same weights.

--parent-lib: a libhq.so built from the parent commit.  Its device-resident C3 step, plain and
under an all-ones mask, is timed in processes of its own alternating with this tree's (parent,
new, new, parent); each new process median is accepted when it lies within the parent's own
process-to-process spread of its neighbouring parent median.
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
from hybrid_timing import load_lib  # noqa: E402
from mask_timing import K, P, SIZE  # noqa: E402


def _set(m, what, np):
    """nothing | ones_mask | weights_<c>"""
    if what == "ones_mask":
        m.setMask(np.ones((SIZE, SIZE), np.uint8))
    elif what.startswith("weights_"):
        m.setWeights(np.full((SIZE, SIZE), int(what.split("_")[1]), np.uint8))
    else:
        m.setMask(None)
    m.setOption("mask_skip", 0 if what != "nothing" else 1)


def child_price(args):
    import numpy as np

    hq, _lib, lib, m = mask_timing._context()
    pals, out = mask_timing._palettes(), {}
    for form, heavy in (("packed", "weights_255"), ("planar", "weights_127")):
        m.setOption("img_u8", 1 if form == "packed" else 0)
        res = {}
        for name, what in (("plain", "nothing"), ("all_ones_mask_no_skip", "ones_mask"), (heavy + "_no_skip", heavy),
                           ("plain_again", "nothing")):
            _set(m, what, np)
            res[name] = mask_timing._measure(args, hq, _lib, lib, m, pals)
            res[name]["w_full"] = m.weightsInfo()[0]
        assert res["plain"]["costs"] == res["all_ones_mask_no_skip"]["costs"]  # bit for bit
        out[form] = res
    m.close()
    print("RESULT " + json.dumps(out))


def child_skip(args):
    import numpy as np

    hq, _lib, lib, m = mask_timing._context()
    side = SIZE // 2
    lo = (SIZE - side) // 2
    wmap = np.zeros((SIZE, SIZE), np.uint8)
    wmap[lo:lo + side, lo:lo + side] = 255
    m.setWeights(wmap)
    pals, out = mask_timing._palettes(), {"region": f"rows and columns [{lo}, {lo + side}) weigh 255, the rest 0",
                                         "area_fraction": side * side / SIZE ** 2}
    for skip in (1, 0, 1):
        m.setOption("mask_skip", skip)
        out[f"mask_skip_{skip}" + ("_again" if f"mask_skip_{skip}" in out else "")] = \
            mask_timing._measure(args, hq, _lib, lib, m, pals)
    m.close()
    assert out["mask_skip_1"]["costs"] == out["mask_skip_0"]["costs"]  # bit for bit
    print("RESULT " + json.dumps(out))


def child_wide(args):
    """The K > 256 form of the sums kernel (16-bit indices, global atomics straight away): its
    `centroid` stage at 4096^2, K = 1024, P = 1 on the packed image, bracketed like `price`."""
    import numpy as np

    hq, _lib, lib, m = mask_timing._context()
    Kw = 1024
    pals = np.random.default_rng(Kw).random((1, 4 * Kw), np.float32)
    pals[:, 3::4] = 0.0
    lib.hq_profile_enable(m.ctx, 1)
    out = {"shape": f"{SIZE}x{SIZE}, K={Kw}, P=1, packed image: centroid_kernel<uint16_t, packed>"}
    for name, what in (("plain", "nothing"), ("all_ones_mask", "ones_mask"), ("weights_255", "weights_255"),
                       ("plain_again", "nothing")):
        _set(m, what, np)
        reps = []
        for i in range(args.warmup + args.reps):
            m.computeQuantizationErrorPopulation(pals, 2.0)
            lib.hq_profile_reset(m.ctx)
            m.clusterSums(1, Kw)
            ms, n = C.c_double(), C.c_int64()
            _lib.check(lib.hq_profile_get(m.ctx, b"centroid", C.byref(ms), C.byref(n)), m.ctx)
            if i >= args.warmup and n.value:
                reps.append(round(ms.value / n.value, 5))
        out[name] = {"centroid_ms_per_launch": statistics.median(reps), "centroid_ms_per_launch_reps": reps}
    m.close()
    print("RESULT " + json.dumps(out))


def child_step(args):
    """The device-resident C3 step of the library at --lib (or this tree's), plain or under an all-ones mask."""
    import numpy as np
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = load_lib(args.lib) if args.lib else hq.load()
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    R, G, B = synthetic_planes(SIZE, SIZE, 1)
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), SIZE, SIZE,
                                             _lib.fptr(sp.illuminant), 0, SIZE), m.ctx)
    m.w = m.h = SIZE
    if args.map == "ones_mask":
        m.setMask(np.ones((SIZE, SIZE), np.uint8))
    params = hq.SWASA(population=P, imax=10 ** 7, seed=1).params()
    h, ran = C.c_void_p(), C.c_int()
    _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, 1, C.byref(h)), m.ctx)

    def run():
        t0 = time.perf_counter()
        _lib.check(lib.hq_search_run(h, args.step_iters, C.byref(ran)), m.ctx)
        dt = time.perf_counter() - t0
        assert ran.value == args.step_iters
        return dt * 1e3 / args.step_iters

    for _ in range(args.step_warmup):
        run()
    reps = [round(run(), 5) for _ in range(args.step_reps)]
    lib.hq_search_destroy(h)
    m.close()
    print("RESULT " + json.dumps({"lib": args.lib or "this tree", "map": args.map, "ms_per_iteration_reps": reps}))


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
    wmap = np.where(which == 0, 255, 1).astype(np.uint8).reshape(h, w)
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)

    def search(**kw):
        sw = hq.SWASA(population=3, imax=60, seed=17)
        best = m.findBestQuantization(rgba.reshape(-1), None, w, Kq, sw, None, None, sp.illuminant, iterations=60,
                                      lloydEvery=1, **kw)
        return np.asarray(best, np.float32), m.bestError, sw.delta

    pw, ew, delta = search(weights=wmap)
    pu, eu, _ = search()
    m.setWeights(wmap)  # (the unweighted search's setImage left nothing set)
    costs = m.computeQuantizationErrorPopulation(np.stack([pw, pu]), delta)
    m.setWeights(None)
    plain = m.computeQuantizationErrorPopulation(np.stack([pw, pu]), delta)
    m.close()
    print("RESULT " + json.dumps({
        "image": "blob_image(96, 64, seed=11): 5 Gaussian colour blobs; blob 0 weighs 255, the rest 1",
        "blob_0_pixels": int((which == 0).sum()), "settings": "K=8, population 3, seed 17, lloydEvery=1, 60 iterations",
        "weighted_cost_of_weighted_search": float(costs[0]), "weighted_cost_of_unweighted_search": float(costs[1]),
        "unweighted_cost_of_weighted_search": float(plain[0]), "unweighted_cost_of_unweighted_search": float(plain[1]),
        "search_best_error_weighted": ew, "search_best_error_unweighted": eu}))


def run_self(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps),
           "--step-iters", str(args.step_iters), "--step-warmup", str(args.step_warmup),
           "--step-reps", str(args.step_reps), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def _brief(d):
    return {k: (v["stage_ms_per_launch"], v["step_ms_per_iteration"]) for k, v in d.items() if isinstance(v, dict)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds before the profiled ones")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (plain and masked C3 step, A/B)")
    ap.add_argument("--step-iters", type=int, default=200, help="iterations per hq_search_run call")
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weights_c3.json"))
    ap.add_argument("--child", default=None, choices=("price", "skip", "step", "quality", "wide"), help=argparse.SUPPRESS)
    ap.add_argument("--only", default=None, help="run this part alone and merge it into --out (wide)")
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--map", default="nothing", choices=("nothing", "ones_mask"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return {"price": child_price, "skip": child_skip, "step": child_step, "quality": child_quality,
                "wide": child_wide}[args.child](args)
    out = {"shape": f"C3: {SIZE}x{SIZE}, K={K}, P={P}, dE76, 72 dpi / 45 cm",
           "warmup_calls": args.warmup, "reps": args.reps,
           "statistic": "median over reps of the HIP-event time of each stage's launch under hq_profile_*; the "
                        "search step: median over reps of the host time of hq_search_run / iterations",
           "not_measured": "anything on more than one GPU; the 32-bit-index and planar K > 256 forms of the weighted "
                           "centroid kernel"}
    if os.path.exists(args.out):  # (figures made outside this script, the disassembly diff for one, stay)
        with open(args.out) as f:
            out.update({k: v for k, v in json.load(f).items() if k in ("disassembly", "resources", "build")})
    if args.only == "wide":
        with open(args.out) as f:
            out = json.load(f)
        out["centroid_k1024"] = run_self(args, "--child", "wide")
        print("centroid_k1024", json.dumps({k: v["centroid_ms_per_launch"] for k, v in out["centroid_k1024"].items()
                                            if isinstance(v, dict)}), flush=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    if args.parent_lib:  # first, on a fresh device
        for what in ("nothing", "ones_mask"):
            ab = {"parent": [], "new": []}
            for name in ("parent", "new", "new", "parent"):
                extra = ["--lib", os.path.abspath(args.parent_lib)] if name == "parent" else []
                ab[name].append(run_self(args, "--child", "step", "--map", what, *extra)["ms_per_iteration_reps"])
            pm = {k: [statistics.median(run) for run in v] for k, v in ab.items()}
            floor = abs(pm["parent"][0] - pm["parent"][1])
            key = "plain_step_vs_parent" if what == "nothing" else "all_ones_mask_step_vs_parent"
            out[key] = {"shape": "C3, packed image, device-resident search, host clock around hq_search_run / iterations",
                        "order": "parent, new, new, parent", "iterations_per_call": args.step_iters,
                        "warmup_calls": args.step_warmup, "ms_per_iteration_reps": ab,
                        "process_medians_ms": {k: [round(x, 5) for x in v] for k, v in pm.items()},
                        "parent_spread_ms": round(floor, 5),
                        "accepted": bool(all(abs(n - p) <= floor for n, p in zip(pm["new"], pm["parent"])))}
            print(key, json.dumps({k: out[key][k] for k in ("process_medians_ms", "parent_spread_ms", "accepted")}),
                  flush=True)
    out["price"] = run_self(args, "--child", "price")
    for form, res in out["price"].items():
        print(form, json.dumps(_brief(res)), flush=True)
    out["region_quarter"] = run_self(args, "--child", "skip")
    print("region_quarter", json.dumps({k: (v["tiles_run"], v["tiles_all"], v["stage_ms_per_launch"]["cost"],
                                            v["step_ms_per_iteration"])
                                        for k, v in out["region_quarter"].items() if isinstance(v, dict)}), flush=True)
    out["centroid_k1024"] = run_self(args, "--child", "wide")
    out["quality"] = run_self(args, "--child", "quality")
    print("quality", json.dumps(out["quality"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
