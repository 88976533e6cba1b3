"""Host-side mirror of the reference's ``ImageManipulation`` (IM) backed by libhq.

Method names, argument order and array layouts follow
``src/plugins/dbrasseur/hybridquantization/ImageManipulation.java`` so a caller
of the reference (or its tests) reads the same against this class.  Every
method runs on the GPU through the C ABI of ``include/hq.h``; nothing here
computes pixels on the host.

Layouts (HQ:279-291 ``makeinline``): inline images are ``float32[4*N]`` RGBA /
Lab with ``.w = 0``; palettes are ``float32[4*K]`` (SW:40-52).

Error behaviour: the reference's constructor turns OpenCL failures into
``openCLAvailable = false`` (IM:79-92) and its methods then silently return
zero arrays (IM:392, IM:590, IM:369, IM:797).  This mirror keeps the flag
(``getOpenCLAvailable()``) but raises ``HQUnavailable`` from every compute
method instead of returning zeros.
"""

from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import HQUnavailable, check, dptr, fptr, iptr, load
from .swasa import fixed_colors, initial_population


class deltaETypes:  # IM:20
    CIE76 = _lib.HQ_DE_CIE76
    CIE94 = _lib.HQ_DE_CIE94
    CIEDE2000 = _lib.HQ_DE_CIEDE2000


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class _Rendering(namedtuple("_Rendering", "name method parameter kw error_attr verbose")):
    """A rendering findBestQuantization was asked for: its *Population method with its parameter (a
    strength, the amplitudes) and keywords, the bestError* attribute its cost goes to, and the verbose
    line's format over (parameter, cost)."""

    def population(self, palettes, delta):
        return self.method(palettes, self.parameter, delta, **self.kw)


def pack_filters(filters, absfilters):
    """IM:800-841 ``updateOpenCLFilters`` packing: Ofilters[3][][] -> k1, k2 (T,4), k3, |k3|."""
    T = len(filters[0][0])
    k1 = np.zeros((T, 4), np.float32)
    k2 = np.zeros((T, 4), np.float32)
    for c in range(3):
        k1[:, c] = filters[c][0]
        k2[:, c] = filters[c][1]
    return k1, k2, _f32(filters[0][2]), _f32(absfilters)


class ImageManipulation:
    """IM:19-895 on libhq (one GPU, one stream)."""

    def __init__(self, deltaEType: int = deltaETypes.CIE76, verbose: bool = False,
                 convergence: bool = True, device: int = 0):
        self._lib = load()  # a missing libhq.so raises here: no silent CPU path
        self.verbose = verbose
        self.convergence = convergence
        self.deltaEType = deltaEType
        self.device = int(device)
        self._ctx = C.c_void_p()
        rc = self._lib.hq_create(device, deltaEType, C.byref(self._ctx))
        self.openCLAvailable = rc == _lib.HQ_OK  # IM:54, IM:78
        if rc not in (_lib.HQ_OK, _lib.HQ_ERR_DEVICE):
            check(rc)
        self.openCLFiltersReady = False
        self._filters = None
        self._assign_space = 0  # option "assign_space" as last set through setOption

    # IM:95
    def getOpenCLAvailable(self) -> bool:
        return self.openCLAvailable

    def _require(self):
        if not self.openCLAvailable:
            raise HQUnavailable(_lib.HQ_ERR_DEVICE, "no usable GPU (IM:79-92 condition)")
        return self._ctx

    @property
    def ctx(self):
        return self._require()

    # IM:800
    def updateOpenCLFilters(self, filters, absfilters):
        ctx = self._require()
        k1, k2, k3, ak3 = pack_filters(filters, absfilters)
        check(self._lib.hq_set_filters(ctx, k1.shape[0], fptr(k1), fptr(k2), fptr(k3), fptr(ak3)),
              ctx)
        self._filters = (k1, k2, k3, ak3)
        self.openCLFiltersReady = True

    @property
    def halfSize(self) -> int:  # IM:408
        return (self._filters[0].shape[0] * 4) // 8

    # IM:100
    def RGBtoXYZ(self, R, G, B):
        ctx = self._require()
        R, G, B = _f32(R), _f32(G), _f32(B)
        out = np.zeros(4 * R.shape[0], np.float32)
        check(self._lib.hq_rgb_to_xyz(ctx, fptr(R), fptr(G), fptr(B), R.shape[0], fptr(out)), ctx)
        return out

    # IM:285
    def XYZtoScielab(self, XYZ, filters, absfilters, w, illuminant):
        ctx = self._require()
        if not self.openCLFiltersReady:
            self.updateOpenCLFilters(filters, absfilters)
        XYZ = _f32(XYZ)
        n = XYZ.shape[0] // 4
        lab = np.zeros(4 * n, np.float32)
        il = _f32(illuminant)
        check(self._lib.hq_xyz_to_scielab(ctx, fptr(XYZ), int(w), n // int(w), fptr(il),
                                          fptr(lab)), ctx)
        return lab

    # device-resident image of IM:450-478 (uploaded once per search)
    def setImage(self, rgbInline, labInline, w, illuminant, row_begin=0, row_end=None):
        """hq_set_image_shard: the inline RGBA image of width ``w`` (and its inline S-CIELAB
        ``labInline``, or None: computed on the device) becomes the context's image.
        ``illuminant``: the white point (Xn, Yn, Zn) Opp->Lab divides by, three floats, each
        finite and greater than 0 (Yn need not be 1); it becomes the context's illuminant, read
        by every later evaluation, rendering and search pass.  None keeps the context's current
        illuminant: D65 on a new context, else the one the last successful setImage /
        setImageReduced left.  A component that is NaN, infinite, zero or negative raises HQError
        (HQ_ERR_ARG, the message names the component) and nothing of the context changes."""
        ctx = self._require()
        rgb = _f32(rgbInline)
        n = rgb.shape[0] // 4
        h = n // int(w)
        lab = _f32(labInline) if labInline is not None else None
        il = None if illuminant is None else _f32(illuminant)
        row_end = h if row_end is None else row_end
        check(self._lib.hq_set_image_shard(ctx, fptr(rgb), fptr(lab) if lab is not None else None,
                                           int(w), h, None if il is None else fptr(il), int(row_begin),
                                           int(row_end)),
              ctx)
        self.w, self.h = int(w), h

    def getLabRef(self):
        ctx = self._require()
        out = np.zeros(4 * self.w * self.h, np.float32)
        check(self._lib.hq_get_labref(ctx, fptr(out)), ctx)
        return out

    def getImage(self):
        """hq_get_image: the device image as the argmin sees it, inline RGBA float32[4 w h]
        with .w = 0 (pairs with getLabRef)."""
        ctx = self._require()
        out = np.zeros(4 * self.w * self.h, np.float32)
        check(self._lib.hq_get_image(ctx, fptr(out)), ctx)
        return out

    # an image pyramid on the device: libhq's additions (hq_set_image_reduced & co.)
    @staticmethod
    def reducedSize(w: int, h: int, factor: int):
        """hq_reduced_size -> (ceil(w / factor), ceil(h / factor)); factor in 1 .. 16."""
        rw, rh = C.c_int(), C.c_int()
        check(load().hq_reduced_size(int(w), int(h), int(factor), C.byref(rw), C.byref(rh)))
        return rw.value, rh.value

    @staticmethod
    def reduceWeights(src, w: int, factor: int, is_mask: bool = False):
        """hq_reduce_weights: a mask (``is_mask``: non-zero counts as 255) or weight map of a
        w-wide image, (h, w) or flat, integer or bool, values 0 .. 255 -> the uint8 (rh, rw)
        weight map of the image reduced by ``factor``: the rounded mean of each block, raised
        to 1 where any byte of the block is non-zero."""
        m = np.asarray(src)
        if m.dtype != np.bool_ and not np.issubdtype(m.dtype, np.integer):
            raise ValueError(f"map of dtype {m.dtype}: an integer or bool array")
        w = int(w)
        if m.ndim not in (1, 2) or w < 1 or m.size == 0 or m.size % w or (m.ndim == 2 and m.shape[1] != w):
            raise ValueError(f"map of shape {m.shape} for an image of width {w}")
        if m.dtype != np.bool_ and (int(m.min()) < 0 or int(m.max()) > 255):
            raise ValueError(f"map values in {int(m.min())} .. {int(m.max())}: bytes, 0 .. 255")
        m = np.ascontiguousarray(m.reshape(-1), dtype=np.uint8)
        h = m.size // w
        rw, rh = ImageManipulation.reducedSize(w, h, factor)
        out = np.zeros((rh, rw), np.uint8)
        check(load().hq_reduce_weights(_lib.u8ptr(m), w, h, int(factor), int(bool(is_mask)), _lib.u8ptr(out)))
        return out

    def setImageReduced(self, src, factor: int, illuminant=None):
        """hq_set_image_reduced: this context's image becomes the box reduction by ``factor`` of
        the image the ImageManipulation ``src`` holds, made on the device; S-CIELAB is computed
        here under this context's own filters.  ``illuminant`` None means ``src``'s.  Mask and
        weights are dropped, as by setImage."""
        ctx = self._require()
        il = None if illuminant is None else _f32(illuminant)
        check(self._lib.hq_set_image_reduced(ctx, src._require(), int(factor), None if il is None else fptr(il)), ctx)
        self.w, self.h = self.reducedSize(src.w, src.h, factor)

    @staticmethod
    def _population(colors):
        """colors: (P, 4K) or list of float[4K] palettes -> (a float32 (P, 4K) array of its own, P, K)."""
        pal = _f32(np.stack([np.asarray(c, np.float32).reshape(-1) for c in colors]))
        return pal, pal.shape[0], pal.shape[1] // 4

    @staticmethod
    def _outputs(P, K, partial=False):
        """A population call's outputs: (costs (P,), used (P, K)), or ``partial`` the (P, 1 + K) rows."""
        return np.zeros((P, 1 + K), np.float64) if partial else (np.zeros(P, np.float64), np.zeros((P, K), np.int32))

    # IM:620 computeQuantizationErrorPopulation
    def computeQuantizationErrorPopulation(self, colors, delta: float = 2.0, return_used=False):
        """colors: (P, 4K) or list of float[4K] palettes -> costs (P,) [, used (P, K)]."""
        return self._populationCall(self._lib.hq_eval_population, colors, (), delta, return_used)

    def _populationCall(self, fn, colors, mid, delta=None, return_used=False):
        """fn(ctx, palettes, P, K, *mid, delta, costs, used) -> costs (P,) [, used (P, K)]; delta None, a
        _partial entry point: fn(ctx, palettes, P, K, *mid, partial) -> the (P, 1 + K) rows.  ``mid`` may be
        a callable, made once the palettes are stacked; a float32 array in it goes as its pointer."""
        ctx = self._require()
        pal, P, K = self._population(colors)
        held = mid() if callable(mid) else mid  # (alive until the call has returned)
        mid = [fptr(x) if isinstance(x, np.ndarray) else x for x in held]
        if delta is None:
            part = self._outputs(P, K, partial=True)
            check(fn(ctx, fptr(pal), P, K, *mid, dptr(part)), ctx)
            return part
        costs, used = self._outputs(P, K)
        check(fn(ctx, fptr(pal), P, K, *mid, float(delta), dptr(costs), iptr(used)), ctx)
        return (costs, used) if return_used else costs

    def getIndices(self, p: int = 0):
        """u8 palette index per pixel of palette p of the last population (K <= 256)."""
        ctx = self._require()
        out = np.zeros(self.w * self.h, np.uint8)
        check(self._lib.hq_get_indices(ctx, int(p), out.ctypes.data_as(_lib._u8)), ctx)
        return out

    def getPixelErrors(self, p: int = 0):
        """Per-pixel dE of palette p of the last population over the owned rows (the
        error image of IM:663-667); needs setOption("pixel_err", 1) before it."""
        ctx = self._require()
        out = np.zeros(self.w * self.h, np.float32)
        check(self._lib.hq_get_pixel_errors(ctx, int(p), fptr(out)), ctx)
        return out

    def getIndices32(self, p: int = 0):
        """32-bit palette index per pixel of palette p of the last population (any K,
        the int index of CL:172-193)."""
        ctx = self._require()
        out = np.zeros(self.w * self.h, np.uint32)
        check(self._lib.hq_get_indices32(ctx, int(p), out.ctypes.data_as(C.POINTER(C.c_uint32))), ctx)
        return out

    # k-means refinement: libhq's additions (hq_cluster_sums & co., no reference counterpart)
    def clusterSums(self, P: int, K: int):
        """Per palette and colour of the last evaluated population: the exact sum of the
        assigned pixels over the owned rows and their count -> (sums int64 (P, K, 4)
        = (sum R, sum G, sum B, count) in units of 1/den, den = 255 or 2**32)."""
        ctx = self._require()
        sums = np.zeros((int(P), int(K), 4), np.int64)
        den = C.c_int64()
        check(self._lib.hq_cluster_sums(ctx, int(P), int(K), _lib.i64ptr(sums), C.byref(den)), ctx)
        return sums, den.value

    @staticmethod
    def centroidsFromSums(sums, den, palettes):
        """The k-means update of hq_centroids_from_sums: palettes (P, 4K) float32 with
        every colour that has pixels replaced by their mean (.w = 0); the others keep
        their bits.  Returns a new array."""
        sums = np.ascontiguousarray(sums, dtype=np.int64)
        P, K = sums.shape[0], sums.shape[1]
        pal = _f32(palettes).reshape(P, 4 * K).copy()
        check(load().hq_centroids_from_sums(_lib.i64ptr(sums), int(den), P, K, fptr(pal)))
        return pal

    def refinePopulation(self, colors, steps, delta: float = 2.0, keep_best=True, return_trace=False):
        """hq_refine_population: `steps` k-means steps on each palette of colors (P, 4K).
        Returns (palettes (P, 4K), costs (P,), used (P, K)) [, trace (steps + 1, P)]."""
        return self._improve(self._lib.hq_refine_population, colors, steps, (float(delta), int(bool(keep_best))),
                             return_trace)

    def _improve(self, fn, colors, steps, mid, return_trace):
        """hq_refine_population's and hq_repair_population's call: fn(ctx, palettes, P, K, steps, *mid, costs,
        used, trace)."""
        ctx = self._require()
        pal, P, K = self._population(colors)
        costs, used = self._outputs(P, K)
        trace = np.zeros((int(steps) + 1, P), np.float64)
        check(fn(ctx, fptr(pal), P, K, int(steps), *mid, dptr(costs), iptr(used), dptr(trace)), ctx)
        return (pal, costs, used, trace) if return_trace else (pal, costs, used)

    # repairing unused colours: libhq's additions (hq_cluster_errors & co., no reference counterpart)
    def clusterErrors(self, P: int, K: int):
        """Per palette and colour of the last population evaluated with option
        "pixel_err" 1: (err int64 (P, K, 4) = (sum of llrint(dE 2**20), count, bits of
        the worst movable pixel's dE, its position y w + x or -1), worst float32
        (P, K, 4) = that pixel's (R, G, B, 0))."""
        ctx = self._require()
        err = np.zeros((int(P), int(K), 4), np.int64)
        worst = np.zeros((int(P), int(K), 4), np.float32)
        check(self._lib.hq_cluster_errors(ctx, int(P), int(K), _lib.i64ptr(err), fptr(worst)), ctx)
        return err, worst

    @staticmethod
    def reseedUnused(err, worst, palettes, max_moves=-1, nfixed=0):
        """The repair rule of hq_reseed_unused: palettes (P, 4K) float32 with every unused
        colour moved onto the worst pixel of the clusters with the most error (at most
        max_moves per palette, < 0: no limit).  ``nfixed`` (hq_reseed_unused_fixed): the first
        nfixed colours of every palette are fixed -- never receivers, donors like any other.
        Returns (a new array, moved (P,))."""
        err = np.ascontiguousarray(err, dtype=np.int64)
        P, K = err.shape[0], err.shape[1]
        worst = np.ascontiguousarray(worst, dtype=np.float32).reshape(P, K, 4)
        pal = _f32(palettes).reshape(P, 4 * K).copy()
        moved = np.zeros(P, np.int32)
        check(load().hq_reseed_unused_fixed(_lib.i64ptr(err), fptr(worst), P, K, int(max_moves), int(nfixed),
                                            fptr(pal), moved.ctypes.data_as(C.POINTER(C.c_int))))
        return pal, moved

    def repairPopulation(self, colors, steps, delta: float = 2.0, max_moves=-1, keep_best=True,
                         return_trace=False):
        """hq_repair_population: `steps` repair steps on each palette of colors (P, 4K).
        Returns (palettes (P, 4K), costs (P,), used (P, K)) [, trace (steps + 1, P)]."""
        return self._improve(self._lib.hq_repair_population, colors, steps,
                             (float(delta), int(max_moves), int(bool(keep_best))), return_trace)

    # dithered rendering: libhq's addition (hq_dither_population, no reference counterpart)
    @staticmethod
    def diffusionPreset(name):
        """hq_diffusion_preset: the diffusion kernel ``name`` ("floyd_steinberg", "jarvis", "stucki",
        "burkes", "sierra3", "sierra2", "sierra_lite", "atkinson") -> (w int32 (3, 5), div): w[dy, dx + 2]
        / div is the share of its error a pixel sends to (x + dx, y + dy)."""
        if name not in _lib.DIFFUSION_PRESETS:
            raise ValueError(f"diffusion kernel {name!r}: one of {', '.join(_lib.DIFFUSION_PRESETS)}")
        t = _lib.hq_diffusion_taps()
        check(load().hq_diffusion_preset(_lib.DIFFUSION_PRESETS.index(name), C.byref(t)))
        return np.array([list(row) for row in t.w], np.int32), int(t.div)

    @classmethod
    def _taps(cls, kernel):
        """``kernel=``: a preset's name or (3 x 5 array of integers, div) -> hq_diffusion_taps."""
        w, div = cls.diffusionPreset(kernel) if isinstance(kernel, str) else kernel
        w = np.asarray(w)
        if w.shape != (3, 5) or not np.all(w == np.round(w)) or int(div) != div:
            raise ValueError("kernel: a preset name or (3 x 5 array of integers, div)")
        if np.any(np.abs(w.astype(np.float64)) >= 2.0 ** 31) or not abs(int(div)) < 2 ** 31:
            raise ValueError("kernel: weights and div are 32-bit integers")
        t = _lib.hq_diffusion_taps()
        for dy in range(3):
            for i in range(5):
                t.w[dy][i] = int(w[dy, i])
        t.div = int(div)
        return t

    def ditherPopulation(self, colors, strength: float = 1.0, delta: float = 2.0, return_used=False, kernel=None):
        """computeQuantizationErrorPopulation of the Floyd-Steinberg rendering at ``strength``
        in [0, 1] (0: the plain evaluation, bit for bit): colors (P, 4K), K <= 256 ->
        costs (P,) [, used (P, K)].  getIndices and getPixelErrors then answer for the
        dithered rendering; clusterSums and clusterErrors need a plain evaluation again.
        ``kernel`` (hq_diffuse_population): another diffusion kernel, a preset's name
        (diffusionPreset) or (3 x 5 array, div); None is hq_dither_population."""
        self._require()
        fn, mid = ((self._lib.hq_dither_population, ()) if kernel is None else
                   (self._lib.hq_diffuse_population, (C.byref(self._taps(kernel)),)))
        return self._populationCall(fn, colors, mid + (float(strength),), delta, return_used)

    def quantizeDithered(self, colors, strength: float = 1.0, kernel=None):
        """The dithered rendering of the context's image (setImage, findBestQuantization)
        with the palette colors float[4K]: ``quantize``'s output format, an inline float4
        image palette[idx] with .w = 0, the indices read back from the device and gathered
        on the host.  Sets ``lastUsedColors`` and ``ditherError``, the rendering's mean dE.
        ``kernel``: ditherPopulation's."""
        return self._quantizeRendered(
            colors, lambda p: self.ditherPopulation(p, strength, 0.0, return_used=True, kernel=kernel), "ditherError")

    def _quantizeRendered(self, colors, population_call, error_attr):
        """The three quantize* renderings' body: population_call(pal (1, 4K)) -> (costs, used)
        renders on the device; its cost goes to the attribute ``error_attr``."""
        pal = _f32(colors).reshape(1, -1)
        costs, used = population_call(pal)
        table = pal.reshape(-1, 4).copy()
        table[:, 3] = 0.0
        self.lastUsedColors = used[0]
        setattr(self, error_attr, float(costs[0]))
        return table[self.getIndices(0)].reshape(-1)

    # dot diffusion: libhq's addition (hq_dot_population, no reference counterpart)
    @staticmethod
    def diffusionClasses(which="knuth8"):
        """hq_dot_preset: the class matrix ``which`` ("knuth8", Knuth's 8 x 8) -> int32 (n, n);
        cls[y, x] is the class of the pixels (x mod n, y mod n)."""
        if which not in _lib.DOT_PRESETS:
            raise ValueError(f"class matrix {which!r}: one of {', '.join(_lib.DOT_PRESETS)}")
        m = _lib.hq_dot_classes()
        check(load().hq_dot_preset(_lib.DOT_PRESETS.index(which), C.byref(m)))
        return np.array(m.cls[:m.n * m.n], np.int32).reshape(m.n, m.n)

    @classmethod
    def _classes(cls, classes):
        """``classes=``: a preset's name or a square integer array -> hq_dot_classes (the
        library judges whether it is legal)."""
        a = cls.diffusionClasses(classes) if isinstance(classes, str) else np.asarray(classes)
        if a.ndim != 2 or a.shape[0] != a.shape[1] or not 1 <= a.shape[0] <= 16 or not np.all(a == np.round(a)):
            raise ValueError("classes: a preset name or a square integer array of side 4, 8 or 16")
        if np.any(np.abs(a.astype(np.float64)) >= 2.0 ** 31):
            raise ValueError("classes: 32-bit integers")
        m = _lib.hq_dot_classes()
        m.n = a.shape[0]
        for i, v in enumerate(a.reshape(-1)):
            m.cls[i] = int(v)
        return m

    def dotPopulation(self, colors, strength: float = 1.0, delta: float = 2.0, classes=None, return_used=False):
        """computeQuantizationErrorPopulation of the dot-diffused rendering (Knuth's dot
        diffusion, one parallel step per class) at ``strength`` in [0, 1] (0: the plain
        evaluation, bit for bit): colors (P, 4K), K <= 256 -> costs (P,) [, used (P, K)].
        ``classes``: the class matrix, a preset's name (diffusionClasses) or a square array of
        side 4, 8 or 16 holding a permutation of 0 .. n*n - 1; None is Knuth's 8 x 8.
        getIndices and getPixelErrors then answer for this rendering; clusterSums and
        clusterErrors need a plain evaluation again."""
        self._require()
        mid = (None if classes is None else C.byref(self._classes(classes)), float(strength))
        return self._populationCall(self._lib.hq_dot_population, colors, mid, delta, return_used)

    def quantizeDotDiffused(self, colors, strength: float = 1.0, classes=None):
        """The dot-diffused rendering of the context's image with the palette colors float[4K],
        in ``quantize``'s output format (quantizeDithered's way).  Sets ``lastUsedColors`` and
        ``dotError``, the rendering's mean dE.  ``classes``: dotPopulation's."""
        return self._quantizeRendered(
            colors, lambda pal: self.dotPopulation(pal, strength, 0.0, classes=classes, return_used=True), "dotError")

    @classmethod
    def dotReach(cls, classes=None):
        """hq_dot_reach: (above, below), the largest number of rows by which a pixel that a
        pixel's dot-diffused index depends on can lie above and below it under the class matrix
        ``classes`` (dotPopulation's; None is Knuth's 8 x 8: (5, 5)).  What a row-block shard
        keeps beyond its extended rows for dotPopulationPartial: setOption("dot_apron", n) with
        n >= both, before setImage(..., row_begin, row_end)."""
        m = cls._classes("knuth8" if classes is None else classes)
        above, below = C.c_int(0), C.c_int(0)
        check(load().hq_dot_reach(C.byref(m), C.byref(above), C.byref(below)))
        return above.value, below.value

    @classmethod
    def dotReach2(cls, classes=None):
        """hq_dot_reach2: (above, below, left, right), dotReach's rows and the same for columns:
        how far around a tile the tiled form of dot diffusion renders (None: Knuth's 8 x 8,
        (5, 5, 5, 5))."""
        m = cls._classes("knuth8" if classes is None else classes)
        v = [C.c_int(0) for _ in range(4)]
        check(load().hq_dot_reach2(C.byref(m), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @classmethod
    def dotLevels(cls, classes=None):
        """hq_dot_levels: (level int32 (n, n), depth): each cell's level -- 0 without a neighbour
        of lower class on the torus, else 1 + the largest level among those -- and the number of
        levels (None: Knuth's 8 x 8, 15 levels)."""
        m = cls._classes("knuth8" if classes is None else classes)
        level, depth = np.zeros(256, np.int32), C.c_int(0)
        check(load().hq_dot_levels(C.byref(m), level.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(depth)))
        return level[:m.n * m.n].reshape(m.n, m.n).copy(), depth.value

    def dotForm(self):
        """hq_dot_form: (form, tile_w, tile_h, levels) of the last dot-diffused pass on this
        context: form 0 none yet, 1 the chain of one launch per class, 2 the tiled kernel
        (option "dot_tile"); the tile is (0, 0) for the chain."""
        return self._values(self._lib.hq_dot_form, 4)

    def dotApron(self):
        """hq_dot_apron: (above, below), the image rows this context holds beyond its extended
        rows on each side (option "dot_apron" when the shard was set, clipped at the image's
        border; (0, 0) on a whole image)."""
        return self._values(self._lib.hq_dot_apron, 2)

    def _values(self, fn, n, ctype=C.c_int):
        """fn(ctx, n pointers to ctype) -> the n values it wrote."""
        ctx = self._require()
        v = [ctype() for _ in range(n)]
        check(fn(ctx, *[C.byref(x) for x in v]), ctx)
        return tuple(x.value for x in v)

    def dotPopulationPartial(self, colors, strength: float = 1.0, classes=None):
        """hq_dot_population_partial: the shard-local (P, 1 + K) partial rows of the dot-diffused
        rendering -- column 0 the dE sum over the owned rows, then the used flags of the extended
        rows.  The partials of disjoint shards of one image add up to the whole image's, the flags
        OR, and each shard's getIndices are the whole image's rows, bit for bit.  A row-block
        shard must hold an apron of at least dotReach(classes) rows on each side (or up to the
        image's border); the sum across shards or ranks is the caller's."""
        self._require()
        mid = (None if classes is None else C.byref(self._classes(classes)), float(strength))
        return self._populationCall(self._lib.hq_dot_population_partial, colors, mid)

    # ordered dithering: libhq's addition (hq_ordered_population, no reference counterpart)
    @staticmethod
    def bayerMap(log2n: int):
        """hq_bayer_map: the Bayer threshold map of side 2**log2n (0 .. 6), float32 (n, n),
        values (B + 0.5) / n**2 - 0.5 for the ranks B = 0 .. n**2 - 1."""
        n = 1 << int(log2n) if 0 <= int(log2n) <= 6 else 1
        m = np.zeros((n, n), np.float32)
        check(load().hq_bayer_map(int(log2n), fptr(m)))
        return m

    @staticmethod
    def orderedAmplitude(K: int) -> float:
        """A starting amplitude for K colours: min(1, 1 / (K**(1/3) - 1)), the spacing of a
        uniform K-colour lattice in the unit cube.  A heuristic, not a tuned value: real
        palettes are not lattices, and on noisy images the best amplitude is lower."""
        side = float(K) ** (1.0 / 3.0) - 1.0
        return 1.0 if side <= 1.0 else 1.0 / side

    def setDitherMap(self, map=None):
        """hq_set_dither_map: the context's threshold map, a 2-D array (mh, mw) with each
        side a power of two up to 64 and values in [-0.5, 0.5]; None restores the default,
        Bayer 16 x 16."""
        ctx = self._require()
        if map is None:
            check(self._lib.hq_set_dither_map(ctx, None, 0, 0), ctx)
            return
        m = np.ascontiguousarray(map, dtype=np.float32)
        if m.ndim != 2:
            raise ValueError(f"map of shape {m.shape}: a 2-D array (rows, columns)")
        check(self._lib.hq_set_dither_map(ctx, fptr(m), m.shape[1], m.shape[0]), ctx)

    @staticmethod
    def _amp3(amp):
        a = np.asarray(amp, np.float32).reshape(-1)
        if a.size == 1:
            a = np.repeat(a, 3)
        if a.size != 3:
            raise ValueError(f"amp={amp!r}: a float or three floats")
        return np.ascontiguousarray(a)

    def orderedPopulation(self, colors, amp, delta: float = 2.0, return_used=False):
        """computeQuantizationErrorPopulation of the ordered-dither rendering: the argmin sees
        each pixel plus ``amp`` (a float, or one per channel, in [0, 1]) times the threshold
        map at its position.  colors (P, 4K), K <= 256 -> costs (P,) [, used (P, K)]; amp 0 is
        the plain evaluation, bit for bit.  getIndices and getPixelErrors then answer for this
        rendering; clusterSums and clusterErrors need a plain evaluation again."""
        return self._populationCall(self._lib.hq_ordered_population, colors, lambda: (self._amp3(amp),), delta,
                                    return_used)

    def orderedPopulationPartial(self, colors, amp):
        """hq_ordered_population_partial: the shard-local (P, 1 + K) partial rows."""
        return self._populationCall(self._lib.hq_ordered_population_partial, colors, lambda: (self._amp3(amp),))

    def quantizeOrdered(self, colors, amp):
        """The ordered-dither rendering of the context's image with the palette colors
        float[4K], in ``quantize``'s output format (quantizeDithered's way).  Sets
        ``lastUsedColors`` and ``orderedError``, the rendering's mean dE."""
        return self._quantizeRendered(
            colors, lambda pal: self.orderedPopulation(pal, amp, 0.0, return_used=True), "orderedError")

    # a pixel mask on the cost: libhq's addition (hq_set_mask, no reference counterpart)
    def setMask(self, mask=None):
        """hq_set_mask: restrict what every cost, clusterSums and colorHistogram measure to
        the pixels where ``mask`` is non-zero -- an (h, w) or flat array of the FULL image, any
        integer or bool dtype.  None clears it.  The image must be set first (setImage drops
        the mask); indices, used flags and stored per-pixel errors do not depend on it."""
        ctx = self._require()
        if mask is None:
            check(self._lib.hq_set_mask(ctx, None, 0, 0), ctx)
            return
        m, w, h = self._pixelMap(mask, "mask")
        m = np.ascontiguousarray((m != 0).reshape(-1), dtype=np.uint8)
        check(self._lib.hq_set_mask(ctx, _lib.u8ptr(m), w, h), ctx)

    def _pixelMap(self, src, noun):
        """setMask's and setWeights' argument as an array of the image's shape -> (it, w, h)."""
        m = np.asarray(src)
        if m.dtype != np.bool_ and not np.issubdtype(m.dtype, np.integer):
            raise ValueError(f"{noun} of dtype {m.dtype}: an integer or bool array")
        if m.ndim not in (1, 2):
            raise ValueError(f"{noun} of shape {m.shape}: (h, w) or flat")
        w, h = getattr(self, "w", 0), getattr(self, "h", 0)
        if (m.ndim == 2 and m.shape != (h, w)) or m.size != w * h:
            raise ValueError(f"{noun} of shape {m.shape} on an image of {h} x {w}")
        return m, w, h

    def maskInfo(self):
        """hq_mask_info -> (n_full, n_owned, tiles_run, tiles_all): the in-mask pixels of the
        full image (w h without a mask) and of the owned rows, and the output tiles per palette
        the last evaluation's fast cost pass launched / would launch without a mask (0, 0 when
        it took the generic path)."""
        return self._values(self._lib.hq_mask_info, 4, C.c_int64)

    # pixel weights on the cost: libhq's addition (hq_set_weights, no reference counterpart)
    def setWeights(self, weights=None):
        """hq_set_weights: weigh every pixel's error by ``weights`` -- an (h, w) or flat array of
        the FULL image, any integer or bool dtype, values 0 .. 255 (0: the pixel is left out).
        Every cost becomes sum(w dE) / sum(w); clusterSums and colorHistogram weigh their sums
        and counts the same way, so k-means moves and the median-cut seed follow the map.  None
        clears it.  Mask and weights are one piece of state: the last of setMask / setWeights
        wins, and setImage drops it.  A float dtype, a value outside 0 .. 255 or a wrong shape is
        a ValueError.  Refused under weights as under a mask: palette slices, clusterErrors and
        the repair moves; on a planar (non-8-bit) image clusterSums, colorHistogram and hybrid
        iterations also need the owned rows' weights to sum to less than 2**31."""
        ctx = self._require()
        if weights is None:
            check(self._lib.hq_set_weights(ctx, None, 0, 0), ctx)
            return
        m, w, h = self._pixelMap(weights, "weights")
        if m.size and (int(m.min()) < 0 or int(m.max()) > 255):
            raise ValueError(f"weights in {int(m.min())} .. {int(m.max())}: bytes, 0 .. 255")
        m = np.ascontiguousarray(m.reshape(-1), dtype=np.uint8)
        check(self._lib.hq_set_weights(ctx, _lib.u8ptr(m), w, h), ctx)

    # fixed palette colours: libhq's addition (hq_set_fixed_colors, no reference counterpart)
    def setFixedColors(self, colors=None):
        """hq_set_fixed_colors: the first n colours of every palette are ``colors`` -- (n, 3),
        (n, 4) or flat 4n, values in [0, 1] -- and no move of a search created from now on, and
        no polish called from now on, changes them.  None (or n = 0) clears them.  A property of
        the context: setImage, setMask and setWeights keep it.  ValueError: a bad shape or a
        value that is not finite or outside [0, 1]."""
        ctx = self._require()
        fx = np.ascontiguousarray(fixed_colors(colors))
        check(self._lib.hq_set_fixed_colors(ctx, fptr(fx) if fx.shape[0] else None, fx.shape[0]), ctx)

    def fixedColors(self):
        """hq_fixed_colors: the context's fixed colours, float32 (n, 4) with .w = 0 ((0, 4): none)."""
        ctx = self._require()
        n = C.c_int()
        check(self._lib.hq_fixed_colors(ctx, C.byref(n), None), ctx)
        out = np.zeros((n.value, 4), np.float32)
        if n.value:
            check(self._lib.hq_fixed_colors(ctx, None, fptr(out)), ctx)
        return out

    def lastPath(self) -> dict:
        """hq_last_path as a dict with names, not numbers: the kernels the last pass enqueued on
        this context took (an evaluation's, a rendering's, the last one of a refine, repair or
        search call).  ``pass``, ``pixels``, ``grid``, ``argmin``, ``cost``, ``cost_instance``,
        ``gen_h`` and ``gen_v`` are strings ("none" before the first pass), ``why_not_fast`` a
        frozenset of reasons (empty on the fast path), everything else an int."""
        ctx = self._require()
        pi = _lib.hq_path_info()
        pi.size = C.sizeof(pi)
        check(self._lib.hq_last_path(ctx, C.byref(pi)), ctx)
        out = {}
        for name, _ in pi._fields_[1:]:
            v = getattr(pi, name)
            key = "pass" if name == "pass_" else name
            if name in _lib.PATH_NAMES:
                out[key] = _lib.PATH_NAMES[name][v]
            elif name == "why_not_fast":
                out[key] = frozenset(n for i, n in enumerate(_lib.PATH_WHY) if v >> i & 1)
            else:
                out[key] = int(v)
        return out

    def searchInfo(self, search) -> dict:
        """hq_search_info of a search handle made on this context: ``device_resident`` (the
        iterations run on the device, not through the host-driven driver), ``nch`` (its chunks
        per palette) and ``graph`` (its last run was captured into a hipGraph)."""
        v = [C.c_int() for _ in range(3)]
        check(self._lib.hq_search_info(search, *[C.byref(x) for x in v]), self._require())
        return {"device_resident": bool(v[0].value), "nch": v[1].value, "graph": bool(v[2].value)}

    def searchPopulation(self, search, P: int, K: int):
        """hq_search_population of a search handle made on this context with a population of P
        palettes of K colours -> (colors float32 (P, 4K), errors float64 (P,)): the members the
        next iteration moves, in the search's order, and each one's error as the search holds it."""
        colors = np.zeros((int(P), 4 * int(K)), np.float32)
        errors = np.zeros(int(P), np.float64)
        check(self._lib.hq_search_population(search, fptr(colors), dptr(errors)), self._require())
        return colors, errors

    def weightsInfo(self):
        """hq_weights_info -> (w_full, w_owned): the sum of the weights over the full image and
        over the owned rows (under a mask or with nothing set: maskInfo's n_full, n_owned)."""
        return self._values(self._lib.hq_weights_info, 2, C.c_int64)

    # seeding the search from the image: libhq's additions (hq_color_histogram, hq_median_cut)
    def colorHistogram(self, bits: int = 5):
        """Colour histogram of the owned rows of the image set: (cells int64
        (2**(3 bits), 4) = (sum R, sum G, sum B, count) per cell (r << 2 bits) | (g << bits) | b
        in units of 1/den, den = 255 or 2**32 as clusterSums')."""
        ctx = self._require()
        cells = np.zeros((1 << (3 * int(bits)) if 2 <= int(bits) <= 6 else 1, 4), np.int64)
        den = C.c_int64()
        check(self._lib.hq_color_histogram(ctx, int(bits), _lib.i64ptr(cells), C.byref(den)), ctx)
        return cells, den.value

    @staticmethod
    def medianCut(cells, bits, den, K):
        """hq_median_cut: the deterministic median cut of such a histogram to K colours ->
        (palette float32[4K], made): colour i < made is the mean of box i's pixels, the
        colours from made on repeat them (fewer non-empty cells than K)."""
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        if not 2 <= int(bits) <= 6 or cells.size != 4 << (3 * int(bits)):
            raise _lib.HQError(_lib.HQ_ERR_ARG, f"bits={bits} with {cells.size // 4} cells")
        pal = np.zeros(4 * max(int(K), 1), np.float32)
        made = C.c_int()
        check(load().hq_median_cut(_lib.i64ptr(cells), int(bits), int(den), int(K), fptr(pal), C.byref(made)))
        return pal, made.value

    # the space of the nearest-colour rule: libhq's addition (option "assign_space", hq_assign_coords)
    ASSIGN_SPACES = ("rgb", "lab")

    @classmethod
    def assignSpaceValue(cls, name) -> int:
        """``assignSpace=``: "rgb" or "lab" -> option "assign_space"'s value; anything else is a ValueError."""
        if not isinstance(name, str) or name not in cls.ASSIGN_SPACES:
            raise ValueError(f"assignSpace={name!r}: one of {', '.join(map(repr, cls.ASSIGN_SPACES))}")
        return cls.ASSIGN_SPACES.index(name)

    @classmethod
    def checkAssignSpace(cls, name, **renderings) -> int:
        """assignSpaceValue, and under "lab" a ValueError naming the renderings asked for with it
        (``renderings``: name -> value; off when None, False or a zero strength): they keep the sRGB rule."""
        space = cls.assignSpaceValue(name)
        on = [k for k, v in renderings.items()
              if not (v is None or v is False or (isinstance(v, (int, float)) and float(v) == 0.0))]
        if space and on:
            raise ValueError(f"assignSpace={name!r} with {', '.join(on)}: error diffusion and ordered dithering keep "
                             "the sRGB rule")
        return space

    def assignCoords(self, colors, space="lab"):
        """hq_assign_coords: the coordinates the argmin ranks ``colors`` -- (n, 3), (n, 4) or flat
        4n -- by in ``space`` under the context's illuminant, float32 (n, 4) with .w = 0: "rgb"
        copies R, G, B; "lab" is (L, a + 128, b + 128) / 256 of the colour's CIELAB, made by the
        device function the evaluation itself uses."""
        value = self.assignSpaceValue(space)
        ctx = self._require()
        a = np.asarray(colors, np.float32)
        if a.ndim == 2 and a.shape[1] == 3:
            a = np.concatenate([a, np.zeros((a.shape[0], 1), np.float32)], axis=1)
        if a.size == 0 or a.size % 4 or (a.ndim == 2 and a.shape[1] != 4) or a.ndim > 2:
            raise ValueError(f"colors of shape {np.shape(colors)}: (n, 3), (n, 4) or flat 4n")
        a = np.ascontiguousarray(a.reshape(-1, 4))
        out = np.zeros_like(a)
        check(self._lib.hq_assign_coords(ctx, value, fptr(a), a.shape[0], fptr(out)), ctx)
        return out

    def quantizeAssigned(self, colors, assignSpace="lab"):
        """The nearest-colour rendering of the context's image with the palette colors float[4K]
        under ``assignSpace``, in ``quantize``'s output format: palette[idx] of the index image of
        one evaluation, so the picture is the one that evaluation scored.  Sets ``lastUsedColors``
        and ``assignedError``, its mean dE.  The context's option is back afterwards."""
        value = self.assignSpaceValue(assignSpace)
        pal = _f32(colors).reshape(1, -1)
        before = self._assign_space
        try:
            self.setOption("assign_space", value)
            costs, used = self.computeQuantizationErrorPopulation(pal, 0.0, return_used=True)
            idx = self.getIndices(0) if pal.shape[1] // 4 <= 256 else self.getIndices32(0)
        finally:
            self.setOption("assign_space", before)
        table = pal.reshape(-1, 4).copy()
        table[:, 3] = 0.0
        self.lastUsedColors = used[0]
        self.assignedError = float(costs[0])
        return table[idx].reshape(-1)

    # IM:383
    def findBestQuantization(self, inlinergbOriginal, inlineScielabOriginal, w, nbOfColors,
                             simulatedAnnealing, filters, absfilters, illuminant,
                             iterations=None, stop=None, lloydSteps=0, lloydEvery=0,
                             init=None, initBits=5, repairEvery=0, repairMoves=-1, repairSteps=0,
                             dither=0.0, ditherSearch=False, ordered=None, orderedSearch=False, mask=None,
                             weights=None, fixed=None, ditherKernel=None, dot=0.0, dotSearch=False,
                             dotClasses=None, assignSpace=None):
        """Full SWASA search (IM:383-591) on the GPU; returns bestColors float[4K].

        ``simulatedAnnealing`` is a :class:`~hybridquantization_amd.swasa.SWASA`;
        ``stop`` is an optional callable polled between chunks (IM:499).
        ``lloydSteps`` > 0 (libhq's addition, the k-means half of the hybrid method):
        the best palette is then polished by that many k-means steps, keeping the
        lowest-cost step (hq_refine_population, keep_best); ``bestError`` and the
        returned colours are the polished ones, ``bestErrorSA`` the search's own.
        ``lloydEvery`` > 0 (hq_search_set_lloyd): every iteration whose 1-based count
        is a multiple of it is a hybrid iteration -- each candidate takes one k-means
        move before it is evaluated, inside the search, on the device when the
        search is device-resident.  The two compose.
        ``init`` (hq_search_create_from): None is the reference's random start;
        ``"mediancut"`` starts every member of the population from the median cut of
        the image's colour histogram at ``initBits`` bits per channel (the members
        part at iteration 1, each with its own draws); an array of shape (4K,) or
        (P, 4K) is the start as given.  ``seedColors`` is then the creation's best
        palette and ``seedError`` its cost, before any iteration.  It composes
        with ``lloydEvery`` and ``lloydSteps``.
        ``repairEvery`` > 0 (hq_search_set_repair): every iteration whose 1-based count
        is a multiple of it is a repair iteration -- each candidate's unused colours
        (at most ``repairMoves``, < 0: no limit) move onto the worst pixels of the
        clusters with the most error before it is evaluated, after the k-means move
        when the iteration is hybrid too.  ``repairSteps`` > 0: the best palette is
        polished by that many repair steps (hq_repair_population, keep_best) before
        the k-means polish; ``bestErrorSA`` is the search's own error.
        ``dither`` > 0 (hq_dither_population, a strength up to 1): once the search and its
        polishes are done, the best palette is also evaluated in its Floyd-Steinberg
        rendering; ``bestErrorDithered`` is that cost, ``bestError`` stays the plain one.
        ``ditherSearch`` (needs ``dither`` > 0): the search optimises the dithered cost
        instead, host-driven (SWASA.search_host with ditherPopulation as its evaluator;
        ``stop`` is not polled); ``init`` composes with it, the k-means and repair moves
        do not (ValueError: both start from a nearest-colour assignment).  ``bestError``
        and ``bestErrorDithered`` are then both the dithered cost.
        ``ditherKernel`` (hq_diffuse_population; ditherPopulation's ``kernel``): the diffusion
        kernel of that final rendering and of ``ditherSearch``; None is Floyd-Steinberg.
        ``ordered`` (hq_ordered_population: an amplitude, a float or three, in [0, 1];
        ``orderedAmplitude(K)`` is a starting point): once the search and its polishes are
        done the best palette is also evaluated in its ordered-dither rendering,
        ``bestErrorOrdered``; ``bestError`` stays the plain one.  ``orderedSearch`` (needs
        ``ordered``): the search itself runs under the ordered cost (hq_search_set_ordered,
        device-resident or host-driven as the options say); ``bestError`` and
        ``bestErrorOrdered`` are then both that cost.  The k-means and repair moves do not
        compose with it (the library refuses them).
        ``mask`` (hq_set_mask; setMask's argument): only the pixels where it is non-zero are
        measured.  It is set after the image and applies to the search, the polishes,
        ``init="mediancut"`` (the histogram of the region) and every reported error.  The
        repair moves have no masked form: ``repairEvery`` / ``repairSteps`` with a mask raise
        ValueError before anything runs.
        ``weights`` (hq_set_weights; setWeights' argument, bytes 0 .. 255): every pixel's error
        counts by its weight, in the search, the polishes, ``init="mediancut"`` and every
        reported error, exactly where a mask would apply.  ``mask`` and ``weights`` together,
        or ``weights`` with ``repairEvery`` / ``repairSteps`` (no weighted error statistic),
        raise ValueError before anything runs.
        ``fixed`` (hq_set_fixed_colors; setFixedColors' argument): the first n colours of the
        palette are given and only the others are optimised -- by the search, its k-means and
        repair moves and the polishes after it, which all run under that state; the returned
        palette's first n colours are ``fixed``'s bits.  It is set for this call and the
        context's previous fixed colours are back afterwards, on every way out.  A bad shape, a
        value outside [0, 1] or n > K raise ValueError before anything runs.
        ``init="mediancut"`` under ``fixed`` cuts to K - n colours and puts the fixed ones in
        front (n = K: no cut); the cut does not know about the fixed colours.  An array ``init``
        keeps its meaning, and its first n colours are overwritten by the library.
        ``ditherSearch`` goes through hq_swasa_search_host_fixed.
        ``dot`` > 0 (hq_dot_population, a strength up to 1; not together with ``dither`` or
        ``ordered``): the best palette is also evaluated in its dot-diffused rendering under
        the class matrix ``dotClasses`` (dotPopulation's ``classes``; None is Knuth's 8 x 8):
        ``bestErrorDot``; ``bestError`` stays the plain one.  ``dotSearch`` "device" (needs ``dot`` > 0, no k-means or repair move): the search runs under
        the dot-diffused cost in the library (hq_search_create[_from] + hq_search_set_dot, device-resident
        where the plain search is); ``bestError`` and ``bestErrorDot`` are one dotPopulation evaluation of
        the returned palette.  ``dotSearch`` True (needs ``dot`` > 0):
        the search optimises the dot-diffused cost instead, host-driven through
        hq_swasa_search_host_fixed exactly as ``ditherSearch`` is, with the same exclusions of
        the k-means and repair moves; ``bestError`` and ``bestErrorDot`` are then both that cost.
        ``assignSpace`` (option "assign_space"): None leaves the context's option as the caller
        set it (0, sRGB, on a new context), and no option call is made; "rgb" is the reference's
        nearest colour in sRGB; "lab" assigns every pixel the palette colour nearest in CIELAB under ``illuminant``, in the
        search, its k-means and repair moves (which stay in RGB) and the polishes, and every
        reported error is that assignment's.  "rgb" or "lab" is set for this call and the value
        last set through setOption is back afterwards.  Anything else, or "lab" together with ``dither``, ``dot``,
        ``ordered`` or their searches, raises ValueError before anything runs.
        """
        space = None if assignSpace is None else self.checkAssignSpace(
            assignSpace, dither=dither, ditherSearch=ditherSearch, ordered=ordered, orderedSearch=orderedSearch,
            dot=dot, dotSearch=dotSearch)
        ctx = self._require()
        fx = None if fixed is None else np.ascontiguousarray(fixed_colors(fixed, int(nbOfColors)))
        before = None if fx is None else self.fixedColors()
        space_before = self._assign_space
        try:
            if fx is not None:
                self.setFixedColors(fx)
            if space is not None:
                self.setOption("assign_space", space)
            return self._findBestQuantization(
                inlinergbOriginal, inlineScielabOriginal, w, nbOfColors, simulatedAnnealing, filters, absfilters,
                illuminant, iterations, stop, lloydSteps, lloydEvery, init, initBits, repairEvery, repairMoves,
                repairSteps, dither, ditherSearch, ordered, orderedSearch, mask, weights, fx, ditherKernel,
                dot, dotSearch, dotClasses)
        finally:
            if space is not None:
                self.setOption("assign_space", space_before)
            if before is not None:
                self.setFixedColors(before)

    def _findBestQuantization(self, inlinergbOriginal, inlineScielabOriginal, w, nbOfColors, simulatedAnnealing,
                              filters, absfilters, illuminant, iterations, stop, lloydSteps, lloydEvery, init,
                              initBits, repairEvery, repairMoves, repairSteps, dither, ditherSearch, ordered,
                              orderedSearch, mask, weights, fx, ditherKernel=None, dot=0.0, dotSearch=False,
                              dotClasses=None):
        """findBestQuantization's body; fx: the call's fixed colours (n, 4), already set on the
        context, or None (then whatever the context holds applies, as to any search)."""
        ctx = self._require()
        nfx = 0 if fx is None else fx.shape[0]
        if mask is not None and weights is not None:
            raise ValueError("mask and weights: one piece of state, give one of them")
        for given, noun, adj in ((mask, "mask", "masked"), (weights, "weights", "weighted")):
            if given is not None and (int(repairEvery) != 0 or int(repairSteps) != 0):
                raise ValueError(f"{noun} with repairEvery or repairSteps: no {adj} error statistic")
        amp = None if ordered is None else self._amp3(ordered)
        if orderedSearch and (amp is None or not np.any(amp != 0)):
            raise ValueError("orderedSearch needs a non-zero ordered amplitude")
        if orderedSearch and (int(lloydSteps) != 0 or int(repairSteps) != 0):
            raise ValueError("orderedSearch with a k-means or repair polish")
        dither = float(dither)
        if ditherKernel is not None:
            self._taps(ditherKernel)  # (a bad one raises before anything runs)
        if not 0.0 <= dither <= 1.0:
            raise ValueError(f"dither={dither!r}: a strength in [0, 1]")
        moves = dict(lloydEvery=lloydEvery, repairEvery=repairEvery, lloydSteps=lloydSteps, repairSteps=repairSteps)

        def host_search_ok(flag, strength_name, strength):
            """ditherSearch / dotSearch: its rendering is on, and no k-means or repair move with it."""
            if not strength > 0.0:
                raise ValueError(f"{flag} needs {strength_name} > 0")
            if any(int(v) != 0 for v in moves.values()):
                raise ValueError(f"{flag} with " + ", ".join(k for k, v in moves.items() if int(v) != 0))

        if ditherSearch:
            host_search_ok("ditherSearch", "dither", dither)
        dot = float(dot)
        if dotClasses is not None:
            self._classes(dotClasses)  # (a bad one raises before anything runs)
        if not 0.0 <= dot <= 1.0:
            raise ValueError(f"dot={dot!r}: a strength in [0, 1]")
        if dot > 0.0 and (dither > 0.0 or amp is not None):
            raise ValueError("dot with dither or ordered: one rendering")
        if isinstance(dotSearch, str) and dotSearch != "device":
            raise ValueError(f"dotSearch={dotSearch!r}: False, True or 'device'")
        if dotSearch:
            host_search_ok("dotSearch", "dot", dot)
        dot_device = isinstance(dotSearch, str)  # hq_search_set_dot; True: the Python host loop
        # the renderings asked for, in the order their final errors are reported, and the one the
        # search itself optimises (None: the plain cost)
        sw = simulatedAnnealing
        rendered = [_Rendering(*r) for on, *r in (
            (dither > 0.0, "dither", self.ditherPopulation, dither, dict(kernel=ditherKernel), "bestErrorDithered",
             "Final error, dithered at strength %g : %.5f"),
            (dot > 0.0, "dot", self.dotPopulation, dot, dict(classes=dotClasses), "bestErrorDot",
             "Final error, dot-diffused at strength %g : %.5f"),
            (amp is not None, "ordered", self.orderedPopulation, amp, {}, "bestErrorOrdered",
             "Final error, ordered dither at amplitude %s : %.5f")) if on]
        goal = "dot" if dotSearch else "dither" if ditherSearch else "ordered" if orderedSearch else None
        searched = next((r for r in rendered if r.name == goal), None)
        if not self.openCLFiltersReady:
            self.updateOpenCLFilters(filters, absfilters)
        # Always upload (IM:450-478 does too): an identity cache keyed on id() can
        # match a new array that reuses a freed one's id, or miss an in-place edit,
        # and the upload is small next to a 5000-iteration search.
        self.setImage(inlinergbOriginal, inlineScielabOriginal, w, illuminant)
        if mask is not None:
            self.setMask(mask)
        if weights is not None:
            self.setWeights(weights)
        params = sw.params()
        handle = C.c_void_p()
        K = int(nbOfColors)
        if isinstance(init, str):
            if init != "mediancut":
                raise ValueError(f"init={init!r}: None, 'mediancut' or an array")
            # under fixed colours: the cut makes the K - n free ones, the fixed ones go in front
            init = np.zeros(4 * K, np.float32)
            init[:4 * nfx] = 0.0 if fx is None else fx.reshape(-1)
            if K - nfx > 0:
                cells, den = self.colorHistogram(int(initBits))
                init[4 * nfx:], _ = self.medianCut(cells, int(initBits), den, K - nfx)
        total = params.imax if iterations is None else min(int(iterations), params.imax)
        if ditherSearch or (dotSearch and not dot_device):
            P = params.population
            best, err, _ = sw.search_host(
                K, lambda ps: searched.population(ps.reshape(P, -1), sw.delta), iterations=total,
                initial=None if init is None else initial_population(init, P, K), fixed=fx)
            self.bestError = err
            setattr(self, searched.error_attr, err)
            self.iterations = total
            if self.verbose:
                print("Final error : %.5f" % err)
            return best
        if init is None:
            check(self._lib.hq_search_create(ctx, C.byref(params), K, sw.seed, C.byref(handle)), ctx)
        else:
            pop = initial_population(init, params.population, K)
            check(self._lib.hq_search_create_from(ctx, C.byref(params), K, sw.seed, fptr(pop),
                                                  C.byref(handle)), ctx)
        try:
            if init is not None:
                seed = np.zeros(4 * K, np.float32)
                seed_err = C.c_double()
                check(self._lib.hq_search_best(handle, fptr(seed), C.byref(seed_err), None), ctx)
                self.seedColors, self.seedError = seed, seed_err.value
            if orderedSearch:
                check(self._lib.hq_search_set_ordered(handle, fptr(amp)), ctx)
            if dot_device:
                classes = None if dotClasses is None else C.byref(self._classes(dotClasses))
                check(self._lib.hq_search_set_dot(handle, classes, dot), ctx)
            if int(lloydEvery) != 0:
                check(self._lib.hq_search_set_lloyd(handle, int(lloydEvery)), ctx)
            if int(repairEvery) != 0:
                check(self._lib.hq_search_set_repair(handle, int(repairEvery), int(repairMoves)), ctx)
            done = 0
            while done < total:
                if stop is not None and stop():
                    break
                ran = C.c_int()
                chunk = min(64, total - done)
                check(self._lib.hq_search_run(handle, chunk, C.byref(ran)), ctx)
                done += ran.value
                if ran.value == 0:
                    break
            best = np.zeros(4 * int(nbOfColors), np.float32)
            err = C.c_double()
            it = C.c_int()
            check(self._lib.hq_search_best(handle, fptr(best), C.byref(err), C.byref(it)), ctx)
            self.bestError = err.value
            self.iterations = it.value
            if self.verbose:
                print("Final error : %.5f" % err.value)  # IM:589
        finally:
            self._lib.hq_search_destroy(handle)
        if dot_device:  # one evaluation of the returned palette: bestError and bestErrorDot are that cost
            self.bestError = float(searched.population(best.reshape(1, -1), sw.delta)[0])
        if int(repairSteps) > 0 or int(lloydSteps) > 0:
            self.bestErrorSA = self.bestError
        if int(repairSteps) > 0:
            pal, costs, _ = self.repairPopulation(best.reshape(1, -1), int(repairSteps), sw.delta,
                                                  int(repairMoves), keep_best=True)
            best, self.bestError = pal[0], float(costs[0])
            if self.verbose:
                print("Final error after %d repair steps : %.5f" % (int(repairSteps), self.bestError))
        if int(lloydSteps) > 0:
            pal, costs, _ = self.refinePopulation(best.reshape(1, -1), int(lloydSteps), sw.delta,
                                                  keep_best=True)
            best, self.bestError = pal[0], float(costs[0])
            if self.verbose:
                print("Final error after %d k-means steps : %.5f" % (int(lloydSteps), self.bestError))
        for r in rendered:  # (the searched one, here the ordered: bestError is already its cost)
            err = self.bestError if r is searched else float(r.population(best.reshape(1, -1), sw.delta)[0])
            setattr(self, r.error_attr, err)
            if self.verbose:
                print(r.verbose % (np.asarray(r.parameter).tolist(), err))
        return best

    # IM:770
    def quantize(self, inlineImageRGB, colors):
        ctx = self._require()
        rgb = _f32(inlineImageRGB)
        col = _f32(colors)
        n, K = rgb.shape[0] // 4, col.shape[0] // 4
        out = np.zeros_like(rgb)
        used = np.zeros(K, np.int32)
        check(self._lib.hq_quantize(ctx, fptr(rgb), n, fptr(col), K, fptr(out), iptr(used)), ctx)
        self.lastUsedColors = used
        return out

    # IM:858
    def computeError(self, original, quantized, errorImage=None):
        ctx = self._require()
        a, b = _f32(original), _f32(quantized)
        n = a.shape[0] // 4
        img = np.zeros(4 * n, np.float32)
        mean = C.c_double()
        check(self._lib.hq_compute_error(ctx, fptr(a), fptr(b), n, fptr(img), C.byref(mean)), ctx)
        if errorImage is not None:
            errorImage[:] = img
        return mean.value

    # RCCL row-block sharding
    def initComm(self, nranks: int, rank: int, unique_id: bytes):
        ctx = self._require()
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        check(self._lib.hq_comm_init(ctx, int(nranks), int(rank), buf), ctx)

    def commInfo(self) -> tuple[int, int]:
        """(ranks, this rank) of the context's RCCL communicator as RCCL reports
        them; (0, -1) without one."""
        return self._values(self._lib.hq_comm_info, 2)

    @staticmethod
    def commUniqueId() -> bytes:
        buf = (C.c_ubyte * 128)()
        check(load().hq_comm_unique_id(buf))
        return bytes(buf)

    def setOption(self, name: str, value: int):
        ctx = self._require()
        check(self._lib.hq_set_option(ctx, name.encode(), int(value)), ctx)
        if name == "assign_space":  # (the library has no getter: what findBestQuantization puts back)
            self._assign_space = int(value)

    # IM:265
    def close(self):
        if self._ctx:
            self._lib.hq_destroy(self._ctx)
            self._ctx = C.c_void_p()
            self.openCLAvailable = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
