"""The image pyramid on one MI355X: what the reduction kernels cost against a device-to-device
copy, what a coarse-to-fine search buys against the plain one at equal wall time, and that the
plain C3 step did not move.

    python scripts/pyramid_timing.py [--parent-lib PATH] [--out profiles/pyramid_c3.json]

(a) reduce: 4096^2 at f = 2 and 4, both forms (the synthetic benchmark image is on the k/255
lattice: the packed form; the same image scaled by 0.999: the planar form).  The kernel alone:
HIP events riding on its launch (hq_profile_get "reduce").  The streaming floor: a
device-to-device copy of the same source bytes (64 MiB packed, 192 MiB planar) in the same
process, torch events around Tensor.copy_.  The whole hq_set_image_reduced call against
hq_set_image of the same reduced image from the host: host clock.  Medians of `reps` after
`warmup` untimed calls.

(b) search: the plain search of N iterations against a ((4, N), (2, N), (1, N - N / 16 - N / 4))
pyramid -- the same step budget when a step on an image reduced by f costs f^-2 -- and against
the one alternative, the same pyramid whose finer levels start at t0 / 10.  Both on the synthetic
benchmark image at C3 (K = 256, P = 4) and on the 96 x 64 blob image (K = 12, P = 4), SWASA
defaults but imax = N, seed 1.  Each search in processes of its own, alternating (plain, pyramid,
alternative, alternative, pyramid, plain); in a process every shape is warmed first (each
level's context, filters, image and a short search), then the timed search runs once: a host
clock from the first level's set-up (contexts, filters, reductions: included; the upload of the
full image, common to all: not) to the last hq_search_run, with the best error read every 50
iterations.  Recorded: final costs, wall times, and the wall time at which the pyramid's
full-resolution level first holds a best error at or below the plain search's final one (null:
never).

(c) --parent-lib: the plain C3 step of the parent commit's libhq.so against this tree's in
alternating processes (scripts/weights_timing.py's step child; parent, new, new, parent).
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

import weights_timing  # noqa: E402
from mask_timing import K, P, SIZE  # noqa: E402

CHUNK = 50


def _full_context(scale=None):
    """The synthetic benchmark image at 4096^2 on a context with the 72 dpi filters."""
    import numpy as np
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    R, G, B = synthetic_planes(SIZE, SIZE, 1)
    if scale is not None:
        R, G, B = (np.ascontiguousarray(p * np.float32(scale)) for p in (R, G, B))
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), SIZE, SIZE,
                                             _lib.fptr(sp.illuminant), 0, SIZE), m.ctx)
    m.w = m.h = SIZE
    m.illum = sp.illuminant
    return hq, _lib, lib, m


def child_reduce(args):
    import numpy as np
    import torch

    out = {}
    for form, scale in (("packed", None), ("planar", 0.999)):
        hq, _lib, lib, src = _full_context(scale)
        src.computeQuantizationErrorPopulation(np.zeros((1, 4 * 8), np.float32), 2.0)
        assert src.lastPath()["pixels"] == ("u8" if form == "packed" else "planar")
        nbytes = SIZE * SIZE * (4 if form == "packed" else 12)
        a = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0").random_()
        b = torch.empty_like(a)
        copies = []
        for i in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                copies.append(e0.elapsed_time(e1))
        del a, b
        copy_ms = statistics.median(copies)
        out[form] = {"source_bytes": nbytes, "d2d_copy_ms": round(copy_ms, 5), "d2d_copy_ms_reps": [round(v, 5) for v in copies],
                     "d2d_copy_GBps_read": round(nbytes / copy_ms / 1e6, 1)}
        for f in (2, 4):
            dst = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
            hq.ScielabProcessor(max(1, round(72 / f)), 45.0, hq.Whitepoint.D65, None, dst)
            lib.hq_profile_enable(dst.ctx, 1)
            kern, whole = [], []
            for i in range(args.warmup + args.reps):
                lib.hq_profile_reset(dst.ctx)
                t0 = time.perf_counter()
                dst.setImageReduced(src, f)
                dt = (time.perf_counter() - t0) * 1e3
                ms, n = C.c_double(), C.c_int64()
                _lib.check(lib.hq_profile_get(dst.ctx, b"reduce", C.byref(ms), C.byref(n)), dst.ctx)
                assert n.value == 1
                if i >= args.warmup:
                    kern.append(ms.value)
                    whole.append(dt)
            lib.hq_profile_enable(dst.ctx, 0)
            reduced = dst.getImage()
            host = []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                dst.setImage(reduced, None, dst.w, src.illum)
                if i >= args.warmup:
                    host.append((time.perf_counter() - t0) * 1e3)
            dst.close()
            k = statistics.median(kern)
            out[form][f"f{f}"] = {
                "kernel_ms": round(k, 5), "kernel_ms_reps": [round(v, 5) for v in kern],
                "kernel_over_d2d_copy": round(k / copy_ms, 3),
                "kernel_GBps_read": round(nbytes / k / 1e6, 1),
                "hq_set_image_reduced_ms": round(statistics.median(whole), 3),
                "hq_set_image_of_the_reduced_image_from_the_host_ms": round(statistics.median(host), 3)}
        src.close()
    print("RESULT " + json.dumps(out))


def _blob_image():
    import numpy as np

    w, h = 96, 64
    rng = np.random.default_rng(11)  # tests/test_lloyd_gpu.py's blob_image(96, 64, seed=11)
    centres = rng.integers(40, 216, (5, 3))
    which = rng.integers(0, 5, w * h)
    by = np.clip(np.rint(centres[which] + 12.0 * rng.standard_normal((w * h, 3))), 0, 255)
    rgba = np.zeros((w * h, 4), np.float32)
    rgba[:, :3] = by.astype(np.float32) / np.float32(255)
    return rgba, w


def _levels(kind, n):
    return ((1, n),) if kind == "plain" else ((4, n), (2, n), (1, n - n // 16 - n // 4))


def _search(hq, _lib, lib, full, kind, Ks, n, trace=True):
    """The levels of `kind` on the full-resolution context `full` (image in place), pyramidSearch's
    steps spelt out so that the clock can be read between them -> (final best error, wall s,
    [(wall s, factor, iterations done on the level, best error on the level)], level set-up s)."""
    sw = hq.SWASA(population=P, imax=n, seed=1)
    population, points, setup = None, [], 0.0
    start = time.perf_counter()
    for i, (f, its) in enumerate(_levels(kind, n)):
        t_level = time.perf_counter()
        m = full
        if f > 1:
            m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
            hq.ScielabProcessor(max(1, round(72 / f)), 45.0, hq.Whitepoint.D65, None, m)
            m.setImageReduced(full, f)
        params = sw.params()
        params.imax = max(its, 1)
        if kind == "pyramid_fine_t0" and i > 0:
            params.t0 = sw.t0 / 10
        h, ran, err = C.c_void_p(), C.c_int(), C.c_double()
        _lib.check(lib.hq_search_create_from(m.ctx, C.byref(params), Ks, sw.seed,
                                             None if population is None else _lib.fptr(population), C.byref(h)), m.ctx)
        setup += time.perf_counter() - t_level if f > 1 else 0.0
        done = 0
        while True:
            if trace or done >= its:
                _lib.check(lib.hq_search_best(h, None, C.byref(err), None), m.ctx)
                points.append((round(time.perf_counter() - start, 5), f, done, err.value))
            if done >= its:
                break
            _lib.check(lib.hq_search_run(h, min(CHUNK, its - done), C.byref(ran)), m.ctx)
            done += ran.value
        population, _ = m.searchPopulation(h, P, Ks)
        lib.hq_search_destroy(h)
        if m is not full:
            m.close()
    return err.value, time.perf_counter() - start, points, setup


def child_search(args):
    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    if args.image == "c3":
        hq, _lib, lib, full = _full_context()
        Ks = K
    else:
        lib = hq.load()
        rgba, w = _blob_image()
        full = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
        sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, full)
        full.setImage(rgba.reshape(-1), None, w, sp.illuminant)
        Ks = 12
    _search(hq, _lib, lib, full, args.kind, Ks, 2 * CHUNK, trace=False)  # every shape warm
    err, wall, points, setup = _search(hq, _lib, lib, full, args.kind, Ks, args.search_iters)
    full.close()
    print("RESULT " + json.dumps({"kind": args.kind, "image": args.image, "K": Ks, "levels": _levels(args.kind, args.search_iters),
                                  "final_error": err, "wall_s": round(wall, 5), "level_setup_s": round(setup, 5),
                                  "trace": points}))


def run_self(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps),
           "--step-iters", str(args.step_iters), "--step-warmup", str(args.step_warmup),
           "--step-reps", str(args.step_reps), "--search-iters", str(args.search_iters), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def compare_searches(args, image):
    runs = {"plain": [], "pyramid": [], "pyramid_fine_t0": []}
    for kind in ("plain", "pyramid", "pyramid_fine_t0", "pyramid_fine_t0", "pyramid", "plain"):
        runs[kind].append(run_self(args, "--child", "search", "--kind", kind, "--image", image))
    plain_final = runs["plain"][0]["final_error"]
    assert all(r["final_error"] == plain_final for r in runs["plain"])  # (the search is deterministic)
    out = {"plain_final_error": plain_final,
           "plain_wall_s": [r["wall_s"] for r in runs["plain"]]}
    for kind in ("pyramid", "pyramid_fine_t0"):
        reach = []
        for r in runs[kind]:
            hit = [t for t, f, _, e in r["trace"] if f == 1 and e <= plain_final]
            reach.append(hit[0] if hit else None)
        r0 = runs[kind][0]
        out[kind] = {"levels": r0["levels"], "final_error": r0["final_error"],
                     "level_final_errors_at_their_own_resolution": [
                         [e for _, f, _, e in r0["trace"] if f == lf][-1] for lf, _ in r0["levels"]],
                     "full_level_error_at_creation": [e for _, f, d, e in r0["trace"] if f == 1 and d == 0][0],
                     "wall_s": [r["wall_s"] for r in runs[kind]], "level_setup_s": [r["level_setup_s"] for r in runs[kind]],
                     "wall_s_to_reach_the_plain_final_error": reach,
                     "final_error_minus_plain": r0["final_error"] - plain_final}
    out["plain_trace_wall_s_iterations_error"] = [(t, d, e) for t, _, d, e in runs["plain"][0]["trace"]]
    out["pyramid_trace_wall_s_factor_iterations_error"] = runs["pyramid"][0]["trace"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls before the timed ones")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (the plain C3 step, A/B)")
    ap.add_argument("--step-iters", type=int, default=200, help="iterations per hq_search_run call of the A/B")
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--step-reps", type=int, default=9)
    ap.add_argument("--search-iters", type=int, default=1000, help="N: the plain search's iterations")
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: reduce, c3, blobs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_c3.json"))
    ap.add_argument("--child", default=None, choices=("step", "reduce", "search"), help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--map", default="nothing", help=argparse.SUPPRESS)
    ap.add_argument("--kind", default="plain", help=argparse.SUPPRESS)
    ap.add_argument("--image", default="c3", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return {"step": weights_timing.child_step, "reduce": child_reduce, "search": child_search}[args.child](args)
    skip = set(filter(None, args.skip.split(",")))
    out = {"shape": f"C3: {SIZE}x{SIZE}, K={K}, P={P}, dE76, 72 dpi / 45 cm", "warmup_calls": args.warmup, "reps": args.reps,
           "not_measured": "anything on more than one GPU; factors other than 2 and 4; level schedules other than the "
                           "default and the one alternative (finer levels at t0 / 10); rocprofv3 counters of the "
                           "reduction kernels"}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out.update({k: v for k, v in json.load(f).items() if k in ("resources", "build")})

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if args.parent_lib:  # first, on a fresh device
        ab = {"parent": [], "new": []}
        for name in ("parent", "new", "new", "parent"):
            extra = ["--lib", os.path.abspath(args.parent_lib)] if name == "parent" else []
            ab[name].append(run_self(args, "--child", "step", *extra)["ms_per_iteration_reps"])
        pm = {k: [statistics.median(run) for run in v] for k, v in ab.items()}
        floor = abs(pm["parent"][0] - pm["parent"][1])
        out["plain_step_vs_parent"] = {
            "shape": "C3, packed image, device-resident search, host clock around hq_search_run / iterations",
            "order": "parent, new, new, parent", "iterations_per_call": args.step_iters,
            "warmup_calls": args.step_warmup, "ms_per_iteration_reps": ab,
            "process_medians_ms": {k: [round(x, 5) for x in v] for k, v in pm.items()},
            "parent_spread_ms": round(floor, 5),
            "accepted": bool(all(abs(n - p) <= floor for n, p in zip(pm["new"], pm["parent"]))),
            "new_minus_parent_ms": [round(n - p, 5) for n, p in zip(pm["new"], pm["parent"])]}
        print("plain_step_vs_parent", json.dumps({k: out["plain_step_vs_parent"][k] for k in
                                                  ("process_medians_ms", "parent_spread_ms", "accepted", "new_minus_parent_ms")}), flush=True)
        save()
    if "reduce" not in skip:
        out["reduce"] = run_self(args, "--child", "reduce")
        print("reduce", json.dumps({form: {k: v for k, v in d.items() if not k.endswith("_reps")}
                                    for form, d in out["reduce"].items()}), flush=True)
        save()
    for image in ("c3", "blobs"):
        if image in skip:
            continue
        out[f"search_{image}"] = compare_searches(args, image)
        print(f"search_{image}", json.dumps({k: v for k, v in out[f"search_{image}"].items() if "trace" not in k}), flush=True)
        save()


if __name__ == "__main__":
    main()
