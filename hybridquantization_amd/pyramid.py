"""Coarse-to-fine SWASA search on a device-built image pyramid (libhq's addition, no
reference counterpart).

The cost is a blurred dE, so it changes little when the image is box-reduced and the
S-CIELAB filters are designed for the correspondingly lower dpi, while a step on an image
reduced by f costs about f**2 times less.  :func:`pyramidSearch` runs the early iterations
on reduced images and hands each level's final population to the next finer level:

* the reduced images are made on the device from the full-resolution context's image
  (``ImageManipulation.setImageReduced``, hq_set_image_reduced);
* a mask or weight map is reduced on the host (``reduceWeights``, hq_reduce_weights);
* a level's population is read with hq_search_population and seeds the next level's
  search through hq_search_create_from.

The policy lives here, in Python: the library has no pyramid inside one context or inside
hq_search_run.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, fptr
from .image_manipulation import ImageManipulation
from .scielab_processor import ScielabProcessor, Whitepoint, design_filters
from .swasa import fixed_colors, initial_population


def check_levels(levels):
    """``levels`` as a tuple of (factor, iterations) int pairs.  ValueError unless it is a
    non-empty sequence of pairs with factors in 1 .. 16 that strictly decrease and end in 1,
    and iteration counts >= 0."""
    try:
        out = tuple((int(f), int(n)) for f, n in levels)
        exact = all(f == int(f) and n == int(n) for f, n in levels)
    except (TypeError, ValueError):
        raise ValueError(f"levels={levels!r}: a sequence of (factor, iterations) pairs") from None
    if not out or not exact:
        raise ValueError(f"levels={levels!r}: a non-empty sequence of integer (factor, iterations) pairs")
    factors = [f for f, _ in out]
    if any(not 1 <= f <= 16 for f in factors):
        raise ValueError(f"levels={levels!r}: factors in 1 .. 16")
    if any(a <= b for a, b in zip(factors, factors[1:])) or factors[-1] != 1:
        raise ValueError(f"levels={levels!r}: strictly decreasing factors that end in 1")
    if any(n < 0 for _, n in out):
        raise ValueError(f"levels={levels!r}: iteration counts >= 0")
    return out


def level_dpi(dpi, factor):
    """The dpi a level's filters are designed at: the image reduced by ``factor`` shows
    ``factor`` times fewer pixels per inch at the same viewing distance."""
    return max(1, round(int(dpi) / int(factor)))


def _run_level(m, sw, K, iterations, population, t0, lloydEvery, repairEvery, repairMoves, stop):
    """One level's search on the context ``m`` (image, filters, weights and fixed colours in
    place): ``sw``'s parameters with imax = ``iterations`` (and ``t0``, when given), started
    from ``population`` ((P, 4K), or None: the reference's random start) and run to its end.
    -> (best colours, best error, (best colours, error) at creation, final population (P, 4K),
    iterations run)."""
    lib, ctx = m._lib, m.ctx
    params = sw.params()
    params.imax = max(int(iterations), 1)  # (a level of 0 iterations evaluates its seed and hands it on)
    if t0 is not None:
        params.t0 = float(np.float32(t0))
    handle = C.c_void_p()
    check(lib.hq_search_create_from(ctx, C.byref(params), K, sw.seed, None if population is None else fptr(population),
                                    C.byref(handle)), ctx)
    try:
        seed, seed_err = np.zeros(4 * K, np.float32), C.c_double()
        check(lib.hq_search_best(handle, fptr(seed), C.byref(seed_err), None), ctx)
        if int(lloydEvery) != 0:
            check(lib.hq_search_set_lloyd(handle, int(lloydEvery)), ctx)
        if int(repairEvery) != 0:
            check(lib.hq_search_set_repair(handle, int(repairEvery), int(repairMoves)), ctx)
        done = 0
        while done < int(iterations):
            if stop is not None and stop():
                break
            ran = C.c_int()
            check(lib.hq_search_run(handle, min(64, int(iterations) - done), C.byref(ran)), ctx)
            done += ran.value
            if ran.value == 0:
                break
        best = np.zeros(4 * K, np.float32)
        err = C.c_double()
        check(lib.hq_search_best(handle, fptr(best), C.byref(err), None), ctx)
        pop, _ = m.searchPopulation(handle, params.population, K)
    finally:
        lib.hq_search_destroy(handle)
    return best, err.value, (seed, seed_err.value), pop, done


def pyramidSearch(ip, inlineRGB, w, K, swasa, dpi=72, viewingDistance=45.0, whitepoint=Whitepoint.D65,
                  levels=None, init=None, mask=None, weights=None, fixed=None, lloydEvery=0, initBits=5,
                  repairEvery=0, repairMoves=-1, fineT0=None, stop=None):
    """A coarse-to-fine SWASA search for K colours on the inline RGBA image ``inlineRGB`` of
    width ``w``; returns bestColors float[4K] at full resolution.

    ``ip`` is the full-resolution :class:`ImageManipulation`; it gets the filters designed at
    ``dpi``, ``viewingDistance`` and ``whitepoint`` and the image (its S-CIELAB computed on the
    device), and holds them afterwards, so ``ip.quantize`` and the renderings follow directly.
    ``levels``: (factor, iterations) pairs with strictly decreasing factors that end in 1;
    None is ((4, imax // 2), (2, imax // 4), (1, imax // 4)) of ``swasa``'s imax.  Every level
    coarser than 1 gets an ImageManipulation of its own on ``ip``'s device, closed on every way
    out, with filters designed at ``max(1, round(dpi / factor))`` and the same viewing distance,
    the image ``setImageReduced(ip, factor)`` and the same fixed colours (``fixed``, or those
    ``ip`` holds already); its weights are
    ``reduceWeights`` of ``mask`` or ``weights``.  Options set on ``ip`` are not copied to them.
    Each level is a search of its own under ``swasa``'s parameters and seed with imax replaced
    by the level's iteration count (``fineT0``: the levels after the coarsest start at that
    temperature instead of ``swasa``'s t0).  The coarsest level starts as ``init`` says --
    None (random), ``"mediancut"`` (of that level's image, at ``initBits``; under ``fixed`` as
    in findBestQuantization) or an array (4K,) / (P, 4K) -- and every level's final population
    seeds the next through hq_search_create_from.  A level of 0 iterations evaluates its seed
    and hands it on.  ``lloydEvery``, ``repairEvery`` / ``repairMoves``: the hybrid and repair
    iterations of findBestQuantization, on every level.
    With ``levels=((1, n),)`` this is findBestQuantization(iterations=n) of a ``swasa`` with
    imax = n, bit for bit.

    Sets on ``ip``: ``bestError``, the full-resolution cost of the returned colours;
    ``levelErrors``, each level's best error at its own resolution, coarsest first;
    ``seedError`` and ``seedColors``, the best of the seed population at full resolution, before
    any full-resolution iteration; ``iterations``, the full-resolution iterations run.

    ValueError before anything runs or any context is created: malformed ``levels``; a level
    whose (reduced) image is narrower or lower than its filters' halfSize, or for whose dpi no filters can be designed; ``mask`` together
    with ``weights``; either of them with ``repairEvery`` (no masked error statistic); bad
    ``fixed`` colours; an ``init`` string other than "mediancut".
    """
    lv = check_levels(((4, swasa.imax // 2), (2, swasa.imax // 4), (1, swasa.imax // 4)) if levels is None else levels)
    K, w = int(K), int(w)
    rgb = np.ascontiguousarray(inlineRGB, dtype=np.float32).reshape(-1)
    h = rgb.shape[0] // 4 // w
    if mask is not None and weights is not None:
        raise ValueError("mask and weights: one piece of state, give one of them")
    if (mask is not None or weights is not None) and int(repairEvery) != 0:
        raise ValueError("mask or weights with repairEvery: no masked or weighted error statistic")
    if isinstance(init, str) and init != "mediancut":
        raise ValueError(f"init={init!r}: None, 'mediancut' or an array")
    fx = None if fixed is None else np.ascontiguousarray(fixed_colors(fixed, K))
    nfx = 0 if fx is None else fx.shape[0]
    for f, _ in lv:  # every level's geometry against its own filters, on the host
        try:
            half = design_filters(level_dpi(dpi, f), viewingDistance, whitepoint)[0].shape[0] * 4 // 8
        except _lib.HQError:
            raise ValueError(f"level of factor {f}: no filters can be designed at {level_dpi(dpi, f)} dpi and "
                             f"viewing distance {viewingDistance}") from None
        rw, rh = ImageManipulation.reducedSize(w, h, f)
        if rw < half or rh < half:
            raise ValueError(f"level of factor {f}: its {rw} x {rh} image is smaller than its filters' halfSize {half} "
                             f"(designed at {level_dpi(dpi, f)} dpi)")
    region = mask if mask is not None else weights

    sp = ScielabProcessor(dpi, viewingDistance, whitepoint, None, ip)
    before = None if fx is None else ip.fixedColors()
    try:
        if fx is not None:
            ip.setFixedColors(fx)
        held = ip.fixedColors()  # (fixed's, or what the context held already: every level gets the same)
        ip.setImage(rgb, None, w, sp.illuminant)
        if mask is not None:
            ip.setMask(mask)
        if weights is not None:
            ip.setWeights(weights)
        population, errors = None, []
        for i, (f, n) in enumerate(lv):
            m = ip
            if f > 1:
                m = ImageManipulation(ip.deltaEType, ip.verbose, ip.convergence, device=ip.device)
            try:
                if f > 1:
                    ScielabProcessor(level_dpi(dpi, f), viewingDistance, whitepoint, None, m)
                    m.setImageReduced(ip, f)
                    if region is not None:
                        m.setWeights(ImageManipulation.reduceWeights(region, w, f, is_mask=mask is not None))
                    if held.shape[0]:
                        m.setFixedColors(held)
                if i == 0 and init is not None:
                    start = init
                    if isinstance(init, str):  # the median cut of this level's image, the fixed colours in front
                        start = np.zeros(4 * K, np.float32)
                        start[:4 * nfx] = 0.0 if fx is None else fx.reshape(-1)
                        if K - nfx > 0:
                            cells, den = m.colorHistogram(int(initBits))
                            start[4 * nfx:], _ = m.medianCut(cells, int(initBits), den, K - nfx)
                    population = initial_population(start, swasa.population, K)
                best, err, (seed, seed_err), population, done = _run_level(
                    m, swasa, K, n, population, fineT0 if i > 0 else None, lloydEvery, repairEvery, repairMoves, stop)
                errors.append(err)
                if ip.verbose:
                    print("Level 1/%d (%d x %d): %d iterations, error %.5f -> %.5f" % (f, m.w, m.h, done, seed_err, err))
            finally:
                if m is not ip:
                    m.close()
    finally:
        if before is not None:
            ip.setFixedColors(before)
    ip.bestError, ip.levelErrors, ip.iterations = err, errors, done
    ip.seedColors, ip.seedError = seed, seed_err
    if ip.verbose:
        print("Final error : %.5f" % err)
    return best
