"""What option "assign_space" 1 (CIELAB nearest colour) costs next to 0 (sRGB) at C3
(4096^2, K = 256, P = 4), and what it does to the cost on small images.

    python scripts/assign_space_timing.py [--out profiles/assign_space_c3.json]

One process, one context on the synthetic benchmark image, the two values in alternating
order (0, 1, 1, 0, ...) so that neither always runs first:

  stages   hq_eval_population under hq_profile_*: the "grid", "assign" and "cost" stages per
           evaluation (HIP events carried by the launches).  Under 1 assign runs its planar
           instance on the coordinate planes (12 B per pixel) where 0 reads the packed bytes (4);
  coords   the coordinate kernel ("coords" stage) for the packed and the planar image form,
           each repetition after a fresh hq_set_image, next to a device-to-device copy of the
           source's bytes (hipMemcpyAsync between HIP events);
  grids    the same stages once more per value under option "grid" 32 and 64;
  step     a device-resident search step (host clock around hq_search_run / iterations).

  quality  (no bar: reported) the cost of the same palettes under both values on the 64 x 64
           ramp under the eight cube corners, the 96 x 64 blob image and the 128 x 128 benchmark
           noise image at K = 8 and 16; and the 60-iteration searches of README's table on the
           blob image (plain, lloydEvery=1, init="mediancut"; K = 8, P = 3, seed 17).
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

SIZE, K, P = 4096, 256, 4
STAGES = ("grid", "assign", "cost", "coords")


def order(reps):
    """0, 1, 1, 0, 0, 1, ...: each value `reps` times, neither always first."""
    out = []
    for i in range(reps):
        out += [0, 1] if i % 2 == 0 else [1, 0]
    return out


def stage_ms(lib, m):
    got = {}
    for k in STAGES:
        ms, n = C.c_double(), C.c_int64()
        if lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n)) == 0 and n.value:
            got[k] = (ms.value, n.value)
    return got


def med(v):
    return round(statistics.median(v), 5)


def bench_context(hq, _lib, lib, scale=None):
    import numpy as np

    from bench import synthetic_planes

    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    planes = synthetic_planes(SIZE, SIZE, 1)
    if scale is not None:  # off the k/255 lattice: the planar form
        planes = [np.ascontiguousarray(p * np.float32(scale)) for p in planes]

    def set_image():
        _lib.check(lib.hq_set_image_planar_shard(m.ctx, *[_lib.fptr(p) for p in planes], SIZE, SIZE,
                                                 _lib.fptr(sp.illuminant), 0, SIZE), m.ctx)
        m.w = m.h = SIZE

    set_image()
    m.illum = sp.illuminant
    return m, set_image


def time_stages(args, hq, _lib, lib, m):
    import numpy as np

    rng = np.random.default_rng(1)
    pals = np.zeros((P, K, 4), np.float32)
    pals[:, :, :3] = rng.random((P, K, 3), dtype=np.float32)
    pals = pals.reshape(P, -1)
    res = {0: {k: [] for k in STAGES}, 1: {k: [] for k in STAGES}}
    pixels = {}
    lib.hq_profile_enable(m.ctx, 1)
    for v in (0, 1):  # warm both (and make the coordinates) before anything is timed
        m.setOption("assign_space", v)
        for _ in range(args.warmup):
            m.computeQuantizationErrorPopulation(pals, 2.0)
    for v in order(args.reps):
        m.setOption("assign_space", v)
        lib.hq_profile_reset(m.ctx)
        for _ in range(args.evals):
            m.computeQuantizationErrorPopulation(pals, 2.0)
        pixels[v] = m.lastPath()["pixels"]
        for k, (ms, n) in stage_ms(lib, m).items():
            res[v][k].append(ms / args.evals)
    lib.hq_profile_enable(m.ctx, 0)
    out = {}
    for v in (0, 1):
        out[f"assign_space_{v}"] = {"pixels": pixels[v],
                                    **{f"{k}_ms": med(x) for k, x in res[v].items() if x},
                                    **{f"{k}_ms_reps": [round(t, 5) for t in x] for k, x in res[v].items() if x}}
    out["assign_1_over_0"] = round(out["assign_space_1"]["assign_ms"] / out["assign_space_0"]["assign_ms"], 3)
    return out


def time_grids(args, hq, _lib, lib, m):
    """The same stages per value and grid resolution (option "grid" 32, the default, and 64)."""
    import numpy as np

    rng = np.random.default_rng(1)
    uni = np.zeros((P, K, 4), np.float32)
    uni[:, :, :3] = rng.random((P, K, 3), dtype=np.float32)
    out = {}
    lib.hq_profile_enable(m.ctx, 1)
    for v in (0, 1):
        for grid in (32, 64):
            m.setOption("assign_space", v)
            m.setOption("grid", grid)
            pals = uni.reshape(P, -1)
            for _ in range(args.warmup):
                m.computeQuantizationErrorPopulation(pals, 2.0)
            lib.hq_profile_reset(m.ctx)
            for _ in range(args.evals):
                m.computeQuantizationErrorPopulation(pals, 2.0)
            out[f"assign_space_{v}_grid_{grid}"] = {f"{k}_ms": round(ms / args.evals, 5)
                                                    for k, (ms, n) in stage_ms(lib, m).items() if k != "coords"}
    lib.hq_profile_enable(m.ctx, 0)
    m.setOption("assign_space", 0)
    m.setOption("grid", 32)
    return out


def time_step(args, hq, _lib, lib, m):
    res = {0: [], 1: []}
    for v in order(args.step_reps):
        m.setOption("assign_space", v)
        params = hq.SWASA(population=P, imax=10 ** 7, seed=1).params()
        h = C.c_void_p()
        _lib.check(lib.hq_search_create(m.ctx, C.byref(params), K, 1, C.byref(h)), m.ctx)
        ran = C.c_int()
        for i in range(args.warmup + 3):
            t0 = time.perf_counter()
            _lib.check(lib.hq_search_run(h, args.iters, C.byref(ran)), m.ctx)
            dt = (time.perf_counter() - t0) * 1e3 / args.iters
            if i >= args.warmup:
                res[v].append(dt)
        lib.hq_search_destroy(h)
    m.setOption("assign_space", 0)
    out = {f"assign_space_{v}": {"ms_per_iteration": med(res[v]), "ms_per_iteration_reps": [round(t, 5) for t in res[v]]}
           for v in (0, 1)}
    out["step_1_over_0"] = round(out["assign_space_1"]["ms_per_iteration"] / out["assign_space_0"]["ms_per_iteration"], 4)
    return out


def d2d_copy_ms(nbytes, warmup=3, reps=9):
    """A device-to-device copy of nbytes on the null stream, timed with HIP events (the runtime
    libhq itself is linked against, through ctypes)."""
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    vp = C.c_void_p

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    a, b, e0, e1 = vp(), vp(), vp(), vp()
    ok(hip.hipMalloc(C.byref(a), C.c_size_t(nbytes)))
    ok(hip.hipMalloc(C.byref(b), C.c_size_t(nbytes)))
    ok(hip.hipMemset(a, 1, C.c_size_t(nbytes)))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    out = []
    for i in range(warmup + reps):
        ok(hip.hipEventRecord(e0, vp()))
        ok(hip.hipMemcpyAsync(b, a, C.c_size_t(nbytes), 3, vp()))  # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, vp()))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        if i >= warmup:
            out.append(ms.value)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    hip.hipFree(a)
    hip.hipFree(b)
    return out


def time_coords(args, hq, _lib, lib):
    import numpy as np

    out = {}
    one = np.zeros((1, 4 * 8), np.float32)
    for form, scale in (("packed", None), ("planar", 0.999)):
        m, set_image = bench_context(hq, _lib, lib, scale)
        m.setOption("assign_space", 1)
        lib.hq_profile_enable(m.ctx, 1)
        kern = []
        for i in range(1 + args.coord_reps):
            if i:
                set_image()
            lib.hq_profile_reset(m.ctx)
            m.computeQuantizationErrorPopulation(one, 2.0)
            m.computeQuantizationErrorPopulation(one, 2.0)  # (the second evaluation makes none)
            ms, n = stage_ms(lib, m)["coords"]
            assert n == 1
            if i:
                kern.append(ms)
        m.setOption("assign_space", 0)
        m.computeQuantizationErrorPopulation(one, 2.0)
        assert m.lastPath()["pixels"] == ("u8" if form == "packed" else "planar")
        m.close()
        nbytes = SIZE * SIZE * (4 if form == "packed" else 12)
        copies = d2d_copy_ms(nbytes)
        k, c = statistics.median(kern), statistics.median(copies)
        out[form] = {"source_bytes": nbytes, "written_bytes": SIZE * SIZE * 12, "kernel_ms": round(k, 5),
                     "kernel_ms_reps": [round(t, 5) for t in kern], "d2d_copy_of_the_source_ms": round(c, 5),
                     "d2d_copy_ms_reps": [round(t, 5) for t in copies], "kernel_over_d2d_copy": round(k / c, 3),
                     "kernel_GBps_read_plus_written": round((nbytes + SIZE * SIZE * 12) / k / 1e6, 1)}
    return out


# ---- quality ---------------------------------------------------------------------------------
def blob_image():
    import numpy as np

    w, h = 96, 64
    rng = np.random.default_rng(11)  # tests/test_lloyd_gpu.py's blob_image(96, 64, seed=11)
    centres = rng.integers(40, 216, (5, 3))
    which = rng.integers(0, 5, w * h)
    by = np.clip(np.rint(centres[which] + 12.0 * rng.standard_normal((w * h, 3))), 0, 255)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    return rgba, w


def ramp_image(w=64, h=64):
    import numpy as np

    x = np.arange(w)[None, :].repeat(h, 0)
    y = np.arange(h)[:, None].repeat(w, 1)
    by = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y) * 255) // (w + h - 2)], -1)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.reshape(-1, 3).astype(np.float32) / np.float32(255)
    return rgba, w


def noise_image(n=128):
    import numpy as np

    from bench import synthetic_planes

    rgba = np.zeros((n * n, 4), np.float32)
    rgba[:, :3] = np.stack(synthetic_planes(n, n, 1), -1)
    return rgba, n


def quality(hq):
    import numpy as np

    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    il = sp.illuminant

    def both(pals, delta=2.0):
        got = {}
        for v in (0, 1):
            m.setOption("assign_space", v)
            costs, used = m.computeQuantizationErrorPopulation(pals, delta, return_used=True)
            got[v] = [(round(float(c), 6), int(u.sum())) for c, u in zip(costs, used)]
        m.setOption("assign_space", 0)
        return got

    out = {"same_palettes": {}, "searches_on_the_blob_image": {}}
    corners = np.zeros((8, 4), np.float32)
    for k in range(8):
        corners[k, :3] = [(k >> 2) & 1, (k >> 1) & 1, k & 1]
    rgba, w = ramp_image()
    m.setImage(rgba.reshape(-1), None, w, il)
    g = both(corners.reshape(1, -1))
    out["same_palettes"]["ramp_64x64_cube_corners"] = {"rgb_cost_used": g[0][0], "lab_cost_used": g[1][0]}
    for name, (rgba, w) in (("blobs_96x64", blob_image()), ("noise_128x128", noise_image())):
        m.setImage(rgba.reshape(-1), None, w, il)
        for KK in (8, 16):
            cells, den = m.colorHistogram(5)
            cut, _ = m.medianCut(cells, 5, den, KK)
            rng = np.random.default_rng(100 + KK)
            rnd = np.zeros((3, KK, 4), np.float32)
            rnd[:, :, :3] = rng.random((3, KK, 3), dtype=np.float32)
            pals = np.concatenate([cut.reshape(1, -1), rnd.reshape(3, -1)])
            g = both(pals)
            out["same_palettes"][f"{name}_K{KK}"] = {
                lab: {"rgb_cost_used": g[0][i], "lab_cost_used": g[1][i]}
                for i, lab in enumerate(("mediancut", "random_a", "random_b", "random_c"))}
    rgba, w = blob_image()
    for label, kw in (("plain", {}), ("lloydEvery=1", dict(lloydEvery=1)), ("init=mediancut", dict(init="mediancut"))):
        row = {}
        for space in ("rgb", "lab"):
            sw = hq.SWASA(population=3, imax=60, seed=17)
            best = m.findBestQuantization(rgba.reshape(-1), None, w, 8, sw, None, None, il, iterations=60,
                                          assignSpace=space, **kw)
            row[space] = {"best_error": round(float(m.bestError), 6)}
            # the other rule's cost of the palette this search found
            g = both(np.asarray(best, np.float32).reshape(1, -1))
            row[space]["same_palette_rgb_cost_used"], row[space]["same_palette_lab_cost_used"] = g[0][0], g[1][0]
        out["searches_on_the_blob_image"][label] = row
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6, help="profiled repetitions per value (stages)")
    ap.add_argument("--evals", type=int, default=10, help="evaluations per repetition")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200, help="iterations per hq_search_run call")
    ap.add_argument("--step-reps", type=int, default=4, help="searches per value, three timed runs each")
    ap.add_argument("--coord-reps", type=int, default=5, help="hq_set_image + coordinate kernel per image form")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_space_c3.json"))
    args = ap.parse_args()

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    out = {"shape": f"C3: {SIZE}x{SIZE}, K={K}, P={P}", "order": "one process; values alternate 0, 1, 1, 0, ...",
           "statistic": "medians, every repetition beside them; stage times: HIP events under hq_profile_*, per "
                        "evaluation; step: host clock around hq_search_run / iterations, profiling off"}
    m, _ = bench_context(hq, _lib, lib)
    out["stages"] = time_stages(args, hq, _lib, lib, m)
    print("stages", json.dumps({k: v for k, v in out["stages"].items()}), flush=True)
    out["stages_by_grid"] = time_grids(args, hq, _lib, lib, m)
    print("grids", json.dumps(out["stages_by_grid"]), flush=True)
    out["search_step"] = time_step(args, hq, _lib, lib, m)
    print("step", json.dumps(out["search_step"]), flush=True)
    m.close()
    out["coords_kernel"] = time_coords(args, hq, _lib, lib)
    print("coords", json.dumps(out["coords_kernel"]), flush=True)
    out["quality"] = quality(hq)
    print("quality", json.dumps(out["quality"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
