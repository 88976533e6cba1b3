"""What findBestQuantization and pyramidSearch share: the table of the moves a search can make and
polish with, and the one session with a library search (hq_search_*) from its creation to its
destroy.  Nothing here knows how a driver chooses its start, its parameters or its iteration count.
"""

from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from ._lib import check, fptr

# iterations per hq_search_run call: ``stop`` is polled between such chunks
CHUNK = 64

# A move: the option that makes every so many iterations of a search one of its iterations and the
# one that asks for so many of its steps as a polish afterwards; the library's setter and the options
# that follow the period in its call, each with its type; ImageManipulation's polish method and the
# options that follow (palettes, steps) in its call; what the verbose line calls its steps.
Move = namedtuple("Move", "every steps setter extra polish polish_args noun")
LLOYD = Move("lloydEvery", "lloydSteps", "hq_search_set_lloyd", (), "refinePopulation", ("delta",), "k-means")
REPAIR = Move("repairEvery", "repairSteps", "hq_search_set_repair", (("repairMoves", int),),
              "repairPopulation", ("delta", "repairMoves"), "repair")
DESCEND = Move("descendEvery", "descendSteps", "hq_search_set_descend", (("descendRate", float),),
               "descendPopulation", ("descendRate", "delta"), "descent")
MOVES = (LLOYD, REPAIR, DESCEND)  # the order of the setters, and of the moves inside one iteration
POLISHES = (REPAIR, LLOYD, DESCEND)  # the order of the polishes after a search


def asked(options, kinds=("every", "steps")):
    """The names of the moves' options of ``kinds`` that ``options`` (name -> value) sets to
    other than 0, the periods first, in the table's order."""
    return [getattr(mv, kind) for kind in kinds for mv in MOVES if int(options[getattr(mv, kind)]) != 0]


Found = namedtuple("Found", "best error iterations ran seed population")


def run_search(im, params, seed, K, population, moves, iterations, stop=None, seeded=False, ordered=None, dot=None,
               want_population=False):
    """One search on the ImageManipulation ``im`` (image, filters, mask or weights and fixed colours
    in place) under the hq_swasa_params ``params`` and ``seed``, for K colours, from its creation to
    its destroy, which runs on every way out.

    ``seeded``: the search is created through hq_search_create_from, from ``population`` ((P, 4K), or
    None: the reference's random start), and its best is read before anything else; otherwise through
    hq_search_create.  ``ordered`` (three amplitudes, float32) or ``dot`` ((hq_dot_classes or None,
    strength)): the rendering the search optimises (hq_search_set_ordered, hq_search_set_dot).
    ``moves`` (name -> value): the moves' periods and the options their setters take, set in MOVES'
    order.  Then ``iterations`` iterations in chunks of CHUNK; ``stop`` (a callable or None) is polled
    before each chunk, and a chunk of which nothing ran ends the loop too.

    -> Found: ``best`` float32[4K] and its ``error``; ``iterations``, the library's count; ``ran``, the
    iterations run here; ``seed``, (best colours, error) at creation (None unless ``seeded``);
    ``population``, the final one (P, 4K) (None unless ``want_population``)."""
    lib, ctx = im._lib, im.ctx

    def best_of(count=None):
        colors, err = np.zeros(4 * K, np.float32), C.c_double()
        check(lib.hq_search_best(handle, fptr(colors), C.byref(err), count), ctx)
        return colors, err.value

    handle = C.c_void_p()
    if seeded:
        check(lib.hq_search_create_from(ctx, C.byref(params), K, seed,
                                        None if population is None else fptr(population), C.byref(handle)), ctx)
    else:
        check(lib.hq_search_create(ctx, C.byref(params), K, seed, C.byref(handle)), ctx)
    try:
        first = best_of() if seeded else None
        if ordered is not None:
            check(lib.hq_search_set_ordered(handle, fptr(ordered)), ctx)
        if dot is not None:
            classes, strength = dot
            check(lib.hq_search_set_dot(handle, None if classes is None else C.byref(classes), strength), ctx)
        for mv in MOVES:
            if int(moves[mv.every]) != 0:
                check(getattr(lib, mv.setter)(handle, int(moves[mv.every]), *[t(moves[n]) for n, t in mv.extra]), ctx)
        done = 0
        while done < iterations:
            if stop is not None and stop():
                break
            ran = C.c_int()
            check(lib.hq_search_run(handle, min(CHUNK, iterations - done), C.byref(ran)), ctx)
            done += ran.value
            if ran.value == 0:
                break
        it = C.c_int()
        best, err = best_of(C.byref(it))
        final = im.searchPopulation(handle, params.population, K)[0] if want_population else None
    finally:
        lib.hq_search_destroy(handle)
    return Found(best, err, it.value, done, first, final)
