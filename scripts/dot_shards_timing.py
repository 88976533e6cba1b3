"""What dot diffusion costs on a row-block shard (hq_dot_population_partial: dot_kernel's windowed
instance over the shard's extended rows and the apron the class matrix's reach needs) next to the
whole image's launch chain in the same process, and that neither the whole-image chain nor the
plain SWASA step moved against the parent commit.

    python scripts/dot_shards_timing.py [--parent-lib PATH] [--out profiles/dot_shards_c3.json]

The shard: one process, one context on the synthetic benchmark image at 4096 x 4096, K = 256,
P = 4 random palettes, Knuth's matrix at strength 1.  The whole image first, then the same
context as rank 3 of 8 (owned rows [1536, 2048), extended +- 10, apron 5 + 5: a window of 542
rows), then as an 8-row shard of the same rank (a window of 38 rows: what the 64 launches cost
with next to no pixels under them).  Per form `warmup` untimed and `reps` profiled calls; recorded
per call the HIP-event time of stage "dot" (from the first launch's start to the last one's end),
the host's wall time around the call and the stage table.  The shortfall of the shard against an
eighth of the whole image's chain is split into the redundant rows (30 of 542, at the whole
image's time per row) and the rest, which the 8-row shard's chain bounds from below.  For
scale, hq_eval_population_partial's grid + assign on the same shard.

--parent-lib: a libhq.so built from the parent commit.  The whole-image chain (hq_dot_population,
P = 1 and 4) at the three shapes of profiles/dot_c3.json, and the plain device-resident C3 step
(scripts/repair_timing.py's code), each in four processes alternating that library with this
tree's (parent, new, new, parent); the two-sided rule: |difference of the medians| within the
larger spread between the two process medians of one library.
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

import repair_timing  # noqa: E402
from hybrid_timing import load_lib  # noqa: E402

SHAPES = {"C1": (512, 16), "C2": (1024, 64), "C3": (4096, 256)}  # (in the order they run)
PS = (1, 4)
STAGES = ("dot", "grid", "assign", "cost", "finalize")
SIZE, K, P, HALF, REACH = 4096, 256, 4, 10, 5
SHARD, FLOOR = (1536, 2048), (2040, 2048)


def _open(lib, size, r0, r1, m=None, apron=0):
    from bench import synthetic_planes

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    if m is None:
        m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=0)
        m.sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
        m.planes = synthetic_planes(size, size, 1)
    if apron:
        m.setOption("dot_apron", apron)
    R, G, B = m.planes
    _lib.check(lib.hq_set_image_planar_shard(m.ctx, _lib.fptr(R), _lib.fptr(G), _lib.fptr(B), size, size,
                                             _lib.fptr(m.sp.illuminant), r0, r1), m.ctx)
    m.w = m.h = size  # (what setImage would have noted)
    return m


def _stages(lib, m):
    from hybridquantization_amd import _lib

    got = {}
    for k in STAGES:
        ms, n = C.c_double(), C.c_int64()
        _lib.check(lib.hq_profile_get(m.ctx, k.encode(), C.byref(ms), C.byref(n)), m.ctx)
        if n.value:
            got[k] = round(ms.value, 5)
    return got


def _timed(lib, m, call, args, stage="dot"):
    for _ in range(args.warmup):
        call()
    ms, wall, tab = [], [], {}
    for _ in range(args.reps):
        lib.hq_profile_reset(m.ctx)
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        tab = _stages(lib, m)
        ms.append(tab[stage] if stage in tab else sum(tab.get(k, 0.0) for k in ("grid", "assign")))
    return {"stage_ms": round(statistics.median(ms), 5), "stage_ms_reps": ms,
            "wall_ms": round(statistics.median(wall), 4), "wall_ms_reps": [round(x, 4) for x in wall],
            "stages_ms_last_rep": tab}


def _palettes(n, k):
    import numpy as np

    pals = np.random.default_rng(k).random((n, 4 * k), np.float32)
    pals[:, 3::4] = 0.0
    return pals


def child_chain(args):
    import hybridquantization_amd as hq

    lib = load_lib(args.lib) if args.lib else hq.load()
    size, k = SHAPES[args.child]
    m = _open(lib, size, 0, size)
    lib.hq_profile_enable(m.ctx, 1)
    out = {"shape": args.child, "lib": args.lib or "this tree", "P": {}}
    for n in PS:
        pals = _palettes(n, k)
        out["P"][str(n)] = _timed(lib, m, lambda: m.dotPopulation(pals, 1.0, 2.0), args)
    m.close()
    print("RESULT " + json.dumps(out))


def child_shard(args):
    import numpy as np

    import hybridquantization_amd as hq
    from hybridquantization_amd import _lib

    lib = hq.load()
    pals = _palettes(P, K)
    m = _open(lib, SIZE, 0, SIZE)
    lib.hq_profile_enable(m.ctx, 1)
    out = {"whole": _timed(lib, m, lambda: m.dotPopulationPartial(pals, 1.0), args)}
    whole = m.dotPopulationPartial(pals, 1.0)
    rows = m.getIndices(0).reshape(SIZE, SIZE)[SHARD[0]:SHARD[1]].copy()
    part = np.zeros((P, 1 + K))

    def plain():
        _lib.check(lib.hq_eval_population_partial(m.ctx, _lib.fptr(pals), P, K, _lib.dptr(part)), m.ctx)

    for name, (r0, r1) in (("shard", SHARD), ("floor", FLOOR)):
        _open(lib, SIZE, r0, r1, m, apron=REACH)
        row = _timed(lib, m, lambda: m.dotPopulationPartial(pals, 1.0), args)
        row["owned_rows"] = [r0, r1]
        row["apron_held"] = list(m.dotApron())
        row["window_rows"] = (r1 - r0) + 2 * (HALF + REACH)
        if name == "shard":
            got = m.getIndices(0)[:(r1 - r0) * SIZE].reshape(r1 - r0, SIZE)
            row["indices_equal_the_whole_images_rows"] = bool(np.array_equal(got, rows))
            row["partial_over_whole"] = float(m.dotPopulationPartial(pals, 1.0)[0, 0] / whole[0, 0])
            row["plain_grid_plus_assign"] = _timed(lib, m, plain, args, stage="grid+assign")
        out[name] = row
    m.close()
    w, s, f = out["whole"]["stage_ms"], out["shard"]["stage_ms"], out["floor"]["stage_ms"]
    win = out["shard"]["window_rows"]
    out["analysis"] = {
        "shard_over_whole": round(s / w, 4), "over_one_eighth": round(s / (w / 8), 3),
        "shortfall_ms": round(s - w / 8, 5),
        "redundant_rows_ms": round(w * (win - (SHARD[1] - SHARD[0])) / SIZE, 5),
        "launch_chain_floor_ms": f,
        "note": "redundant_rows_ms: the window's rows beyond the owned ones at the whole image's time per row; "
                "launch_chain_floor_ms: the 64 launches over a 38-row window, the part of a shard's chain that "
                "does not shrink with its rows"}
    print("RESULT " + json.dumps(out))


def run_self(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--warmup", str(args.warmup), "--reps", str(args.reps), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


def two_sided(ab):
    """ab: {"parent": [reps of process 1, of process 2], "new": [...]} -> the rule's figures."""
    med = {k: statistics.median(x for run in v for x in run) for k, v in ab.items()}
    pm = {k: [statistics.median(run) for run in v] for k, v in ab.items()}
    spread = {k: abs(v[0] - v[1]) for k, v in pm.items()}
    return {"reps_ms": ab, "median_ms": {k: round(v, 5) for k, v in med.items()},
            "process_medians_ms": {k: [round(x, 5) for x in v] for k, v in pm.items()},
            "new_minus_parent_ms": round(med["new"] - med["parent"], 5),
            "spread_between_process_medians_ms": {k: round(v, 5) for k, v in spread.items()},
            "within_spread_two_sided": abs(med["new"] - med["parent"]) <= max(spread.values()),
            "new_over_parent": round(med["new"] / med["parent"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls before the profiled ones")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libhq.so of the parent commit (A/B)")
    ap.add_argument("--step-iters", type=int, default=200, help="A/B: iterations per hq_search_run call")
    ap.add_argument("--step-reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dot_shards_c3.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "shard":
        return child_shard(args)
    if args.child is not None:
        return child_chain(args)
    out = {"shard_shape": f"{SIZE}x{SIZE}, K={K}, P={P}, Knuth's 8 x 8 matrix, strength 1, one MI355X; rank 3 of 8",
           "warmup_calls": args.warmup, "reps": args.reps,
           "statistic": "median over reps; stage_ms: HIP events carried by the launches (hq_profile_*: 'dot' from the "
                        "first launch's start to the last one's end); wall_ms: the host clock around the whole call",
           "not_measured": "more than one GPU: the eight ranks side by side, and any exchange of partials"}

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    out["shard"] = run_self(args, "--child", "shard")
    print("shard", json.dumps(out["shard"]["analysis"]), flush=True)
    save()
    if args.parent_lib:
        order = ("parent", "new", "new", "parent")
        out["whole_image_chain_vs_parent"] = {}
        for shape in SHAPES:
            runs = {"parent": [], "new": []}
            for name in order:
                extra = ["--lib", os.path.abspath(args.parent_lib)] if name == "parent" else []
                runs[name].append(run_self(args, "--child", shape, *extra))
            res = {"shape": f"{SHAPES[shape][0]}x{SHAPES[shape][0]}, K={SHAPES[shape][1]}"}
            for n in PS:
                res[f"P={n}"] = two_sided({k: [r["P"][str(n)]["stage_ms_reps"] for r in v] for k, v in runs.items()})
            out["whole_image_chain_vs_parent"][shape] = res
            print(shape, {k: (v["median_ms"], v["within_spread_two_sided"]) for k, v in res.items() if k != "shape"},
                  flush=True)
            save()
        step = argparse.Namespace(iters=args.step_iters, warmup=3, reps=args.step_reps, prof_reps=1, timeout=args.timeout)
        ab = {"parent": [], "new": []}
        for name in order:
            res = repair_timing.run_child(step, "C3", args.parent_lib if name == "parent" else None, plain_only=True)
            ab[name].append(res["device_plain"]["ms_per_iteration_reps"])
        out["plain_step_vs_parent"] = dict(
            shape="C3, device-resident plain search, host clock around hq_search_run / iterations",
            iterations_per_call=args.step_iters, **two_sided(ab))
        print("plain step", out["plain_step_vs_parent"]["median_ms"],
              out["plain_step_vs_parent"]["within_spread_two_sided"], flush=True)
    save()


if __name__ == "__main__":
    main()
