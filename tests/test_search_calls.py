"""The Python search drivers' conversation with the library, without a GPU: findBestQuantization and
pyramidSearch run on an ImageManipulation made without hq_create whose library is a recording stub, and
the calls they make, in order, are compared with literal lists; the refusal rules are walked for their
texts, raised before anything runs.

A recorded call is (name, arguments): of a library call the context ("ctx0": the caller's own, "ctx1"
..: the pyramid's level contexts), ints, floats and None as they were passed, hq_swasa_params as
"imax=.. t0=..", and nothing for a pointer, a handle or an array; of a method stubbed at the Python
level (no image is set, so whatever needs geometry is one) its context and the arguments that matter."""

import numpy as np
import pytest

import hybridquantization_amd as hq
from hybridquantization_amd import _lib
from hybridquantization_amd.pyramid import pyramidSearch

IM = hq.ImageManipulation
W, H, K, SEED = 64, 48, 4, 7
POLISHES = ("hq_repair_population", "hq_refine_population", "hq_descend_population")


class Library:
    """Every entry of the library: records the call and returns 0.  hq_search_run writes
    ran = min(chunk, what is left of the imax the search was created with), or 0 from its
    ``zero_from``-th call on, and raises on its ``fail_at``-th; hq_search_best writes zeros; the n-th
    polish writes cost n; hq_fixed_colors counts what hq_set_fixed_colors last set."""

    def __init__(self, calls, zero_from=None, fail_at=None):
        self.calls, self.zero_from, self.fail_at = calls, zero_from, fail_at
        self.left = self.runs = self.polishes = 0
        self.nfixed = {}

    @staticmethod
    def scalars(args):
        out = []
        for a in args:
            obj = getattr(a, "_obj", None)
            if isinstance(obj, _lib.hq_swasa_params):
                out.append("imax=%d t0=%g" % (obj.imax, obj.t0))
            elif a is None or isinstance(a, (int, float, str)):
                out.append(a)
        return tuple(out)

    def __getattr__(self, name):
        def call(*args):
            # (hq_search_best's pointers are outputs: which of them a caller asks for is not recorded)
            self.calls.append((name, self.scalars(args[:1] if name == "hq_search_best" else args)))
            if name in ("hq_search_create", "hq_search_create_from"):
                self.left = args[1]._obj.imax
            elif name == "hq_search_run":
                self.runs += 1
                if self.fail_at == self.runs:
                    raise RuntimeError("run failed")
                ran = 0 if self.zero_from is not None and self.runs >= self.zero_from else min(args[1], self.left)
                self.left -= ran
                args[2]._obj.value = ran
            elif name in POLISHES:
                self.polishes += 1
                args[-3][0] = float(self.polishes)
            elif name == "hq_set_fixed_colors":
                self.nfixed[args[0]] = args[2]
            elif name == "hq_fixed_colors" and args[1] is not None:
                args[1]._obj.value = self.nfixed.get(args[0], 0)
            return 0
        return call


@pytest.fixture
def stub(monkeypatch):
    """-> make(**Library's options) -> (an ImageManipulation on the stub, the recorded calls); every
    ImageManipulation made afterwards (the pyramid's level contexts) is one on the same stub."""
    calls, made = [], []

    def init(self, deltaEType=0, verbose=False, convergence=True, device=0):
        self._lib, self._ctx = made[0], "ctx%d" % (len(made) - 1)
        self.verbose, self.convergence, self.deltaEType, self.device = verbose, convergence, deltaEType, device
        self.openCLAvailable, self.openCLFiltersReady, self._assign_space = True, False, 0
        self.close = lambda: calls.append(("close", (self._ctx,)))  # (on the instance: __del__ finds it too)
        if len(made) > 1:
            calls.append(("ImageManipulation", (self._ctx,)))
        made.append(self)

    def geometry(name, result, keep=lambda *a: a):
        def method(self, *a, **kw):
            calls.append((name, (self._ctx,) + tuple(keep(*a))))
            return result(self, *a, **kw)
        monkeypatch.setattr(IM, name, method)

    def size(factor):
        def set_size(self, *a, **kw):
            self.w, self.h = IM.reducedSize(W, H, factor(*a))
        return set_size

    geometry("updateOpenCLFilters", lambda self, *a: setattr(self, "openCLFiltersReady", True), lambda *a: ())
    geometry("setImage", size(lambda *a: 1), lambda rgb, lab, w, il: (w,))
    geometry("setImageReduced", size(lambda src, f: f), lambda src, f: (src._ctx, f))
    geometry("colorHistogram", lambda self, bits: ("cells", 255))
    geometry("kmeansppSeed", lambda self, P, K, seed: (np.full((P, 4 * K), 0.25, np.float32), None))
    monkeypatch.setattr(IM, "medianCut", staticmethod(
        lambda cells, bits, den, K: calls.append(("medianCut", (cells, bits, den, K)))
        or (np.full(4 * K, 0.5, np.float32), K)))

    class Processor:
        illuminant = np.ones(3, np.float32)

        def __init__(self, dpi, viewingDistance, whitepoint, HQ=None, imageProcessor=None):
            calls.append(("ScielabProcessor", (imageProcessor._ctx, dpi)))

    monkeypatch.setattr("hybridquantization_amd.pyramid.ScielabProcessor", Processor)
    monkeypatch.setattr(IM, "__init__", init)

    def make(**options):
        made.append(Library(calls, **options))
        return IM(), calls
    return make


def swasa(imax=5, **kw):
    return hq.SWASA(population=2, imax=imax, seed=SEED, **kw)


def find(m, sw, **kw):
    return m.findBestQuantization("rgb", None, W, K, sw, None, None, None, **kw)


def create(imax=5, ctx="ctx0", t0=20):
    return ("hq_search_create", (ctx, "imax=%d t0=%g" % (imax, t0), K, SEED))


def create_from(imax=5, ctx="ctx0", t0=20, start=True):
    return ("hq_search_create_from", (ctx, "imax=%d t0=%g" % (imax, t0), K, SEED) + (() if start else (None,)))


UPLOAD = [("updateOpenCLFilters", ("ctx0",)), ("setImage", ("ctx0", W))]
BEST = ("hq_search_best", ())
RUN5 = ("hq_search_run", (5,))
END = [BEST, ("hq_search_destroy", ())]
FIXED = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]


def test_plain(stub):
    m, calls = stub()
    best = find(m, swasa())
    assert calls == UPLOAD + [create(), RUN5] + END
    assert best.shape == (4 * K,) and m.bestError == 0.0 and m.iterations == 0
    assert not hasattr(m, "bestErrorSA") and not hasattr(m, "seedError")


def test_array_start(stub):
    m, calls = stub()
    find(m, swasa(), init=np.zeros(4 * K, np.float32))
    assert calls == UPLOAD + [create_from(), BEST, RUN5] + END
    assert m.seedError == 0.0 and m.seedColors.shape == (4 * K,)


def test_kmeanspp_start(stub):
    m, calls = stub()
    find(m, swasa(), init="kmeans++")
    assert calls == UPLOAD + [("kmeansppSeed", ("ctx0", 2, K, SEED)), create_from(), BEST, RUN5] + END


def test_median_cut_with_fixed_colours(stub):
    m, calls = stub()
    find(m, swasa(), init="mediancut", fixed=FIXED, initBits=4)
    assert calls == [
        ("hq_fixed_colors", ("ctx0", None)),  # what the context held: nothing
        ("hq_set_fixed_colors", ("ctx0", 2)),
    ] + UPLOAD + [
        ("colorHistogram", ("ctx0", 4)),
        ("medianCut", ("cells", 4, 255, K - 2)),
        create_from(), BEST, RUN5,
    ] + END + [("hq_set_fixed_colors", ("ctx0", None, 0))]


def test_median_cut_with_every_colour_fixed(stub):
    m, calls = stub()
    find(m, swasa(), init="mediancut", fixed=FIXED + FIXED)
    assert [c[0] for c in calls if c[0] in ("colorHistogram", "medianCut")] == []
    assert calls[4:7] == [create_from(), BEST, RUN5]


def test_three_moves_in_the_search(stub):
    m, calls = stub()
    find(m, swasa(), lloydEvery=2, repairEvery=3, repairMoves=1, descendEvery=4, descendRate=0.5)
    assert calls == UPLOAD + [
        create(),
        ("hq_search_set_lloyd", (2,)),
        ("hq_search_set_repair", (3, 1)),
        ("hq_search_set_descend", (4, 0.5)),
        RUN5,
    ] + END
    assert not hasattr(m, "bestErrorSA")


def test_three_polishes(stub):
    m, calls = stub()
    find(m, swasa(), lloydSteps=2, repairSteps=3, repairMoves=1, descendSteps=4)
    assert calls == UPLOAD + [create(), RUN5] + END + [
        ("hq_repair_population", ("ctx0", 1, K, 3, 2.0, 1, 1)),
        ("hq_refine_population", ("ctx0", 1, K, 2, 2.0, 1)),
        ("hq_descend_population", ("ctx0", 1, K, 4, hq.image_manipulation.DESCEND_RATE, 2.0)),
    ]
    assert m.bestErrorSA == 0.0 and m.bestError == 3.0  # the search's own; the last polish's


@pytest.mark.parametrize("polish, entry", zip(("repairSteps", "lloydSteps", "descendSteps"), POLISHES))
def test_one_polish(stub, polish, entry):
    m, calls = stub()
    find(m, swasa(), **{polish: 1})
    assert [c[0] for c in calls[6:]] == [entry]
    assert m.bestErrorSA == 0.0 and m.bestError == 1.0


def test_ordered_search_with_descent(stub):
    m, calls = stub()
    find(m, swasa(), ordered=0.25, orderedSearch=True, descendEvery=2)
    assert calls == UPLOAD + [
        create(),
        ("hq_search_set_ordered", ()),
        ("hq_search_set_descend", (2, hq.image_manipulation.DESCEND_RATE)),
        RUN5,
    ] + END  # (no evaluation after it: bestErrorOrdered is the search's error)
    assert m.bestErrorOrdered == m.bestError == 0.0


def test_dot_search_on_the_device(stub):
    m, calls = stub()
    find(m, swasa(), dot=0.5, dotSearch="device")
    assert calls == UPLOAD + [
        create(),
        ("hq_search_set_dot", (None, 0.5)),
        RUN5,
    ] + END + [("hq_dot_population", ("ctx0", 1, K, None, 0.5, 2.0))]
    assert m.bestErrorDot == m.bestError == 0.0


def test_chunk_loop(stub):
    m, calls = stub()
    polls = []
    find(m, swasa(200), iterations=130, stop=lambda: polls.append(len(calls)) or False)
    assert calls == UPLOAD + [create(200)] + [("hq_search_run", (n,)) for n in (64, 64, 2)] + END
    assert polls == [3, 4, 5]  # before each chunk


def test_chunk_loop_early_stop(stub):
    m, calls = stub()
    find(m, swasa(200), iterations=130, stop=lambda: any(c[0] == "hq_search_run" for c in calls))
    assert calls == UPLOAD + [create(200), ("hq_search_run", (64,))] + END


def test_chunk_loop_nothing_ran(stub):
    m, calls = stub(zero_from=2)
    find(m, swasa(200), iterations=130)
    assert calls == UPLOAD + [create(200), ("hq_search_run", (64,)), ("hq_search_run", (64,))] + END  # (no third)


def test_exception_in_the_loop_reaches_destroy(stub):
    m, calls = stub(fail_at=2)
    with pytest.raises(RuntimeError, match="run failed"):
        find(m, swasa(200), fixed=FIXED)
    assert calls[4:] == [create(200), ("hq_search_run", (64,)), ("hq_search_run", (64,)),
                         ("hq_search_destroy", ()), ("hq_set_fixed_colors", ("ctx0", None, 0))]


def level(ctx, imax, n, t0=20, start=True, sets=()):
    """One level's search as pyramidSearch holds it: always created from a population (None: random),
    the seed's best read, the population read before the destroy."""
    runs = [("hq_search_run", (min(64, n - i),)) for i in range(0, n, 64)]
    return ([create_from(imax, ctx, t0, start), BEST] + list(sets) + runs +
            [BEST, ("hq_search_population", ()), ("hq_search_destroy", ())])


def test_pyramid_one_level(stub):
    m, calls = stub()
    best = pyramidSearch(m, np.zeros(4 * W * H, np.float32), W, K, swasa(), levels=((1, 70),))
    assert calls == [("ScielabProcessor", ("ctx0", 72)), ("hq_fixed_colors", ("ctx0", None)),
                     ("setImage", ("ctx0", W))] + level("ctx0", 70, 70, start=False)
    assert best.shape == (4 * K,) and m.iterations == 70 and m.levelErrors == [0.0] and m.seedError == 0.0


def test_pyramid_no_iterations(stub):
    m, calls = stub()
    pyramidSearch(m, np.zeros(4 * W * H, np.float32), W, K, swasa(), levels=((1, 0),), init=np.zeros(4 * K))
    assert calls[3:] == level("ctx0", 1, 0)  # (imax at least 1; the seed is evaluated and handed on)
    assert m.iterations == 0


def test_pyramid_two_levels_with_moves(stub):
    m, calls = stub()
    sets = [("hq_search_set_lloyd", (2,)), ("hq_search_set_repair", (3, 1)), ("hq_search_set_descend", (4, 0.5))]
    pyramidSearch(m, np.zeros(4 * W * H, np.float32), W, K, swasa(), levels=((2, 3), (1, 4)), init="mediancut",
                  initBits=4, fixed=FIXED, lloydEvery=2, repairEvery=3, repairMoves=1, descendEvery=4,
                  descendRate=0.5, fineT0=5.0)
    assert calls == [
        ("ScielabProcessor", ("ctx0", 72)),
        ("hq_fixed_colors", ("ctx0", None)),  # what the context held: nothing
        ("hq_set_fixed_colors", ("ctx0", 2)),
        ("hq_fixed_colors", ("ctx0", None)), ("hq_fixed_colors", ("ctx0", None)),  # what every level gets
        ("setImage", ("ctx0", W)),
        ("ImageManipulation", ("ctx1",)),
        ("ScielabProcessor", ("ctx1", 36)),
        ("setImageReduced", ("ctx1", "ctx0", 2)),
        ("hq_set_fixed_colors", ("ctx1", 2)),
        ("colorHistogram", ("ctx1", 4)),
        ("medianCut", ("cells", 4, 255, K - 2)),
    ] + level("ctx1", 3, 3, sets=sets) + [("close", ("ctx1",))] + level("ctx0", 4, 4, t0=5, sets=sets) + [
        ("hq_set_fixed_colors", ("ctx0", None, 0)),
    ]
    assert m.iterations == 4 and m.levelErrors == [0.0, 0.0]


def test_pyramid_exception_closes_the_level_and_restores(stub):
    m, calls = stub(fail_at=1)
    with pytest.raises(RuntimeError, match="run failed"):
        pyramidSearch(m, np.zeros(4 * W * H, np.float32), W, K, swasa(), levels=((2, 3), (1, 4)), fixed=FIXED)
    assert calls[-4:] == [("hq_search_run", (3,)), ("hq_search_destroy", ()), ("close", ("ctx1",)),
                          ("hq_set_fixed_colors", ("ctx0", None, 0))]


MASK = np.ones((H, W), np.uint8)
REFUSED = [
    (dict(mask=MASK, weights=MASK), "mask and weights: one piece of state, give one of them"),
    (dict(mask=MASK, repairEvery=2), "mask with repairEvery or repairSteps: no masked error statistic"),
    (dict(weights=MASK, repairSteps=2), "weights with repairEvery or repairSteps: no weighted error statistic"),
    (dict(mask=MASK, descendSteps=2),
     "descendSteps with a mask, weights or a searched rendering: the gradient is the plain cost's"),
    (dict(descendEvery=2, dither=0.5, ditherSearch=True),
     "descendEvery with a mask, weights, ditherSearch or dotSearch: the gradient needs an unmasked cost and an "
     "assign-only pass"),
    (dict(orderedSearch=True), "orderedSearch needs a non-zero ordered amplitude"),
    (dict(ordered=0.0, orderedSearch=True), "orderedSearch needs a non-zero ordered amplitude"),
    (dict(ordered=0.25, orderedSearch=True, lloydSteps=2), "orderedSearch with a k-means or repair polish"),
    (dict(ditherSearch=True), "ditherSearch needs dither > 0"),
    (dict(dither=0.5, ditherSearch=True, lloydEvery=2), "ditherSearch with lloydEvery"),
    (dict(dither=0.5, ditherSearch=True, repairEvery=2, lloydSteps=1), "ditherSearch with repairEvery, lloydSteps"),
    (dict(dot=0.5, dither=0.5), "dot with dither or ordered: one rendering"),
    (dict(dot=0.5, dotSearch="gpu"), "dotSearch='gpu': False, True or 'device'"),
    (dict(dot=0.5, dotSearch=True, repairSteps=1), "dotSearch with repairSteps"),
    # two rules broken: the earlier check's text
    (dict(mask=MASK, repairEvery=2, descendEvery=2), "mask with repairEvery or repairSteps: no masked error statistic"),
    (dict(descendSteps=1, descendEvery=1, dot=0.5, dotSearch=True),
     "descendSteps with a mask, weights or a searched rendering: the gradient is the plain cost's"),
]


@pytest.mark.parametrize("kw, text", REFUSED, ids=[" ".join(kw) for kw, _ in REFUSED])
def test_refused_before_anything_runs(stub, kw, text):
    m, calls = stub()
    with pytest.raises(ValueError) as e:
        find(m, swasa(), **kw)
    assert str(e.value) == text
    assert calls == []


def test_bad_init_string(stub):
    """findBestQuantization learns of a bad ``init`` where it starts the search, after the upload;
    pyramidSearch before anything runs."""
    m, calls = stub()
    with pytest.raises(ValueError) as e:
        find(m, swasa(), init="median")
    assert str(e.value) == "init='median': None, 'mediancut', 'kmeans++' or an array"
    assert calls == UPLOAD
    del calls[:]
    with pytest.raises(ValueError) as e:
        pyramidSearch(m, np.zeros(4 * W * H, np.float32), W, K, swasa(), levels=((1, 4),), init="kmeans++")
    assert str(e.value) == "init='kmeans++': None, 'mediancut' or an array"
    assert calls == []


PYRAMID_REFUSED = [
    (dict(mask=MASK, weights=MASK), "mask and weights: one piece of state, give one of them"),
    (dict(mask=MASK, repairEvery=2), "mask or weights with repairEvery: no masked or weighted error statistic"),
    (dict(mask=MASK, descendEvery=2), "mask or weights with descendEvery: the gradient is the unmasked cost's"),
    (dict(weights=MASK, repairEvery=2, descendEvery=2),
     "mask or weights with repairEvery: no masked or weighted error statistic"),
]


@pytest.mark.parametrize("kw, text", PYRAMID_REFUSED, ids=[" ".join(kw) for kw, _ in PYRAMID_REFUSED])
def test_pyramid_refused_before_any_context(stub, kw, text):
    m, calls = stub()
    with pytest.raises(ValueError) as e:
        pyramidSearch(m, np.zeros(4 * W * H, np.float32), W, K, swasa(), levels=((2, 3), (1, 4)), **kw)
    assert str(e.value) == text
    assert calls == []
