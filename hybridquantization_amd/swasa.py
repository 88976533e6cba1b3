"""Mirror of the reference's ``SWASA`` parameter object (SW:3-116).

The policy itself (RNG, neighbours, acceptance, temperature, convergence) runs
natively inside libhq (hq_swasa.h / hq_host.cpp) so the search loop has no
Python in it.  ``icy.util.Random`` is unseeded in the reference (SW:46); here
the generator is ``java.util.Random``-compatible and seeded explicitly.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, load


def initial_population(init, P: int, K: int) -> np.ndarray:
    """A given start as the (P, 4K) float32 array hq_search_create_from and
    hq_swasa_search_host_from take: (P, 4K) as it is, (4K,) for every member."""
    pop = np.asarray(init, np.float32)
    if pop.shape == (4 * K,):
        pop = np.tile(pop, (P, 1))
    if pop.shape != (P, 4 * K):
        raise ValueError(f"initial population of shape {pop.shape}: want ({4 * K},) or ({P}, {4 * K})")
    return np.ascontiguousarray(pop)


def fixed_colors(fixed, K=None) -> np.ndarray:
    """Fixed palette colours as the (n, 4) float32 array hq_set_fixed_colors takes, .w = 0:
    ``fixed`` is (n, 3), (n, 4) or flat 4n; None or an empty one is n = 0.  ValueError: another
    shape, a value that is not finite or lies outside [0, 1], n > K (K given)."""
    if fixed is None:
        return np.zeros((0, 4), np.float32)
    a = np.asarray(fixed, np.float32)
    if a.ndim == 1 and a.size % 4 == 0:
        a = a.reshape(-1, 4)
    if a.ndim != 2 or a.shape[1] not in (3, 4):
        raise ValueError(f"fixed colours of shape {a.shape}: want (n, 3), (n, 4) or flat 4n")
    out = np.zeros((a.shape[0], 4), np.float32)
    out[:, :3] = a[:, :3]
    if not np.all((out >= 0.0) & (out <= 1.0)):  # (a NaN fails both)
        raise ValueError("fixed colours with a channel that is not finite or outside [0, 1]")
    if K is not None and out.shape[0] > int(K):
        raise ValueError(f"{out.shape[0]} fixed colours in a palette of K = {int(K)}")
    return out


class SWASA:
    """SW:14 ``SWASA(population, imax, iTc, delta, convDelay, convSpread, t0, alpha, s0, beta, HQ)``."""

    def __init__(self, population=4, imax=5000, iTc=20, delta=2.0, convDelay=0.75,
                 convSpread=0.15, t0=20.0, alpha=0.9, s0=100.0, beta=5.3, HQ=None, seed=0,
                 convergence=True):
        self.population = int(population)
        self.imax = int(imax)
        self.iTc = int(iTc)
        self.delta = float(np.float32(delta))
        self.convergenceDelay = float(np.float32(convDelay))
        self.convergenceRate = float(np.float32(convSpread))
        self.t0 = float(np.float32(t0))
        self.alpha = float(np.float32(alpha))
        self.s0 = float(np.float32(s0))
        self.beta = float(np.float32(beta))
        self.plugin = HQ
        self.seed = int(seed)
        self.convergence = bool(convergence)

    def getImax(self):  # SW:36
        return self.imax

    def getPopulationSize(self):  # SW:113
        return self.population

    def params(self) -> _lib.hq_swasa_params:
        return _lib.hq_swasa_params(self.population, self.imax, self.iTc, self.delta,
                                    self.convergenceDelay, self.convergenceRate, self.t0,
                                    self.alpha, self.s0, self.beta, int(self.convergence))

    def computePenalty(self, usedColors) -> float:  # SW:74-82
        return float(np.count_nonzero(np.asarray(usedColors) == 0)) * self.delta

    def search_host(self, K: int, eval_population, iterations=None, refine=None, every=0, initial=None,
                    fixed=None):
        """Run the native SWASA driver with a Python population evaluator.

        eval_population(palettes (P, K, 4) float32) -> costs (P,).  Returns
        (best_colors float[4K], best_error, trace (iterations, 1+P)).  This is
        the hook the CPU tests use to check the policy without a GPU.

        ``refine`` and ``every`` (libhq's addition, hq_swasa_search_host_lloyd): on
        iteration ite with ite % every == 0 the candidates go through
        refine(palettes (P, K, 4) float32) before they are evaluated; it updates
        the array in place or returns the updated palettes.  With ``refine``
        None and ``every`` 0 this is hq_swasa_search_host.

        ``initial`` (libhq's addition, hq_swasa_search_host_from): the population the
        search starts from, (P, 4K) or (4K,) for every member, in place of the
        random one, whose draws are still made.

        ``fixed`` (libhq's addition, hq_swasa_search_host_fixed): the first n colours of every
        palette, (n, 3), (n, 4) or flat 4n (ValueError before anything runs for a bad shape, a
        value outside [0, 1] or n > K).  They are written over every member at the start and no
        iteration changes them, not even ``refine``: the driver puts them back after it.
        """
        lib = load()
        params = self.params()
        iters = self.imax if iterations is None else int(iterations)
        errbox = []
        fx = np.ascontiguousarray(fixed_colors(fixed, K))
        nfx = fx.shape[0]

        def _cb(user, pal, P, KK, costs):
            try:
                arr = np.ctypeslib.as_array(pal, shape=(P * KK * 4,)).reshape(P, KK, 4).copy()
                out = np.asarray(eval_population(arr), dtype=np.float64)
                for i in range(P):
                    costs[i] = float(out[i])
                return 0
            except Exception as e:  # surfaced after the call
                errbox.append(e)
                return 1

        cb = _lib.EVAL_FN(_cb)
        best = np.zeros(4 * K, np.float32)
        err = C.c_double()
        trace = np.zeros(iters * (1 + self.population), np.float64)
        rf = _lib.REFINE_FN()
        if refine is not None:
            def _rf(user, pal, P, KK):
                try:
                    arr = np.ctypeslib.as_array(pal, shape=(P * KK * 4,)).reshape(P, KK, 4)
                    res = refine(arr)  # in place, or the updated palettes
                    if res is not None:
                        arr[...] = np.asarray(res, np.float32).reshape(P, KK, 4)
                    return 0
                except Exception as e:
                    errbox.append(e)
                    return 1

            rf = _lib.REFINE_FN(_rf)
        if nfx > 0:
            pop = None if initial is None else initial_population(initial, self.population, int(K))
            rc = lib.hq_swasa_search_host_fixed(C.byref(params), int(K), self.seed, iters, cb, rf, int(every),
                                                None if pop is None else _lib.fptr(pop),
                                                _lib.fptr(fx), nfx, None,
                                                _lib.fptr(best), C.byref(err), _lib.dptr(trace))
        elif initial is not None:
            pop = initial_population(initial, self.population, int(K))
            rc = lib.hq_swasa_search_host_from(C.byref(params), int(K), self.seed, iters, cb, rf,
                                               int(every), _lib.fptr(pop), None, _lib.fptr(best),
                                               C.byref(err), _lib.dptr(trace))
        elif refine is None and int(every) == 0:
            rc = lib.hq_swasa_search_host(C.byref(params), int(K), self.seed, iters, cb, None,
                                          _lib.fptr(best), C.byref(err), _lib.dptr(trace))
        else:
            rc = lib.hq_swasa_search_host_lloyd(C.byref(params), int(K), self.seed, iters, cb, rf,
                                                int(every), None, _lib.fptr(best), C.byref(err),
                                                _lib.dptr(trace))
        if errbox:
            raise errbox[0]
        check(rc)
        return best, err.value, trace.reshape(iters, 1 + self.population)
