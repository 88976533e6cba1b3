"""GPU tests of the descent move inside the search (hq_search_set_descend, hq_descend_move: libhq's
additions): the device's move against the float64 statement of hq.h on hq_cost_gradient's own
output; one search run four ways, bit for bit; the refusals."""
import dataclasses

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
from hybridquantization_amd import _lib
from test_grad_gpu import FILTERS, context, noise_rgba, palettes
from test_hybrid_gpu import Search
from test_lloyd_gpu import blob_image

pytestmark = pytest.mark.gpu

RATE = np.float32(1e-3)
# (w, h, K, P, palette seed, option grad_tiled, fixed colours, ordered amplitude): 40 x 35 = 2 x 2 tiles
# of 32 x 32 and 2 x 3 of 32 x 16; W = H = halfSize = 10, where both folds reach every pixel; 70 x 67 at
# K = 256 leaves colours unused (palettes()' duplicate at least); one ordered rendering.
MOVES = [(40, 35, 8, 2, 33, 0, 0, None), (40, 35, 8, 2, 33, 1, 0, None), (10, 10, 2, 1, 19, -1, 0, None),
         (70, 67, 256, 1, 276, -1, 2, None), (40, 35, 8, 2, 33, -1, 0, 0.3)]


@pytest.mark.parametrize("w,h,K,P,seed,form,nfixed,amp", MOVES)
def test_move_against_float64(gpu, w, h, K, P, seed, form, nfixed, amp):
    """Every channel within one float32 spacing of clamp(x - rate grad N / n, 0, 1) in float64 (the sums are
    the same integers; the device's pow may differ from the host's in its last bit); colours without pixels
    and fixed colours keep their bits."""
    filt = FILTERS["designed"]()
    m = context(gpu, filt)
    try:
        m.setImage(noise_rgba(w, h, 3).reshape(-1), None, w, filt.illum)
        m.setOption("grad_tiled", form)
        pals = palettes(P, K, seed)
        if nfixed:
            m.setFixedColors(pals[0].reshape(K, 4)[:nfixed])
        if amp is None:
            m.computeQuantizationErrorPopulation(pals, 2.0)
        else:
            m.orderedPopulation(pals, amp, 2.0)
        grad, n = m.costGradient(P, K)
        x = pals.reshape(P, K, 4)[..., :3]
        moves = (n > 0) & (np.arange(K) >= nfixed)
        with np.errstate(divide="ignore", invalid="ignore"):
            step = np.float64(RATE) * grad * (w * h) / n[..., None]
        want = np.where(moves[..., None], np.clip(x.astype(np.float64) - step, 0.0, 1.0), x).astype(np.float32)
        got = m.descendMove(pals, RATE, amp).reshape(P, K, 4)
        off = np.abs(got[..., :3].astype(np.float64) - want) / np.spacing(want)
        print(f"{w}x{h} K={K} form={form}: {int(moves.sum())} of {P * K} colours move, largest move "
              f"{np.abs(want - x).max():.3e}, largest distance {off.max():.2f} spacings")
        assert moves.any() and not moves.all() and np.abs(want - x).max() > 1e-4
        assert (off <= 1.0).all()
        assert got[~moves].tobytes() == pals.reshape(P, K, 4)[~moves].tobytes() and not got[..., 3].any()
    finally:
        m.close()


def run_search(m, K, plan, device=1, graph=0, every=None, lloyd=0, repair=0, amp=None, P=3, seed=17, act=None):
    """A search of 12 iterations in the runs of `plan` -> (best colours' bytes, best error's bytes, iteration)."""
    m.setOption("sa_device", device)
    m.setOption("sa_graph", graph)
    s = Search(m, K, hq.SWASA(population=P, imax=12, seed=seed, t0=0.05))
    try:
        if amp is not None:
            _lib.check(s.lib.hq_search_set_ordered(s.h, _lib.fptr(np.full(3, amp, np.float32))), m.ctx)
        for rc in (s.set_lloyd(lloyd), s.lib.hq_search_set_repair(s.h, repair, -1),
                   _lib.HQ_OK if every is None else s.lib.hq_search_set_descend(s.h, every, RATE)):
            _lib.check(rc, m.ctx)
        assert m.searchDescendInfo(s.h) == (every or 0, RATE if every else 0.0)
        refused = act(m, s) if act else None
        for n in plan:
            s.run(n)
        best, err, it = s.best()
        return (best.tobytes(), np.float64(err).tobytes(), it), (best, err), refused
    finally:
        s.close()


# all3: iterations 6 and 12 of the 12 apply the k-means, repair and descent moves together.  At run_search's
# seed 17 each of the three takes part: the run without any one of them ends on other bytes.
SEARCHES = {"every1": dict(every=1), "every3": dict(every=3), "lloyd2": dict(every=3, lloyd=2),
            "repair2": dict(every=1, repair=2), "ordered": dict(every=1, amp=0.3), "fixed": dict(every=1),
            "all3": dict(every=3, lloyd=2, repair=3)}


@pytest.mark.parametrize("name", SEARCHES)
def test_one_search_four_ways(gpu, name):
    """Device-resident, captured, host-driven and split 7 + 5: the same best colours, error and iteration."""
    kw, K = SEARCHES[name], 8
    filt, (rgba, _) = FILTERS["designed"](), blob_image(96, 64, seed=11)
    m = context(gpu, filt)
    try:
        m.setImage(rgba.reshape(-1), None, 96, filt.illum)
        if name == "fixed":
            m.setFixedColors(o.synthetic_palette(K, 40).reshape(K, 4)[:2])
        dev, (best, err), _ = run_search(m, K, (12,), **kw)
        assert run_search(m, K, (12,), graph=1, **kw)[0] == dev
        assert run_search(m, K, (12,), device=0, **kw)[0] == dev
        assert run_search(m, K, (7, 5), **kw)[0] == dev
        without = run_search(m, K, (12,), **dict(kw, every=0))[0]
        plain = run_search(m, K, (12,), lloyd=kw.get("lloyd", 0), repair=kw.get("repair", 0), amp=kw.get("amp"))
        assert without == plain[0] and dev != without  # every = 0 is the search without the call; the move took part
        again = (m.orderedPopulation(best[None], kw["amp"], 2.0) if "amp" in kw
                 else m.computeQuantizationErrorPopulation(best[None], 2.0))[0]
        print(f"{name}: best {err!r} with the move, {np.frombuffer(without[1])[0]!r} without")
        assert abs(again - err) <= 1e-6 * abs(err)
    finally:
        m.close()


def _set(every=2, rate=RATE):
    return lambda m, s: s.lib.hq_search_set_descend(s.h, every, rate)


def _under(name, value, back):
    """The set call with option `name` at `value`, the option back at `back` afterwards."""
    def act(m, s):
        m.setOption(name, value)
        rc = _set()(m, s)
        m.setOption(name, back)
        return rc
    return act


def _dot_then_set(m, s):
    _lib.check(s.lib.hq_search_set_dot(s.h, None, 1.0), m.ctx)
    return _set()(m, s)


def _set_then_dot(m, s):
    _lib.check(_set(every=100)(m, s), m.ctx)  # (a period no iteration of the run meets)
    return s.lib.hq_search_set_dot(s.h, None, 1.0)


REFUSALS = {
    # name: (dE type, K, what the context is under before the search is created, the refused call, its status)
    "k_above_256": ("CIE76", 300, None, _set(), _lib.HQ_ERR_UNSUPPORTED),
    "de94": ("CIE94", 8, None, _set(), _lib.HQ_ERR_UNSUPPORTED),
    "de2000": ("CIEDE2000", 8, None, _set(), _lib.HQ_ERR_UNSUPPORTED),
    "shard": ("CIE76", 8, "shard", _set(), _lib.HQ_ERR_UNSUPPORTED),
    "slice": ("CIE76", 8, None, _under("slice_ranks", 2, 1), _lib.HQ_ERR_UNSUPPORTED),
    "palette_split": ("CIE76", 8, None, _under("palette_split", 1, 0), _lib.HQ_ERR_UNSUPPORTED),
    "mask": ("CIE76", 8, "mask", _set(), _lib.HQ_ERR_UNSUPPORTED),
    "weights": ("CIE76", 8, "weights", _set(), _lib.HQ_ERR_UNSUPPORTED),
    "taps": ("CIE76", 8, "taps", _set(), _lib.HQ_ERR_UNSUPPORTED),
    "dot_then_descend": ("CIE76", 8, None, _dot_then_set, _lib.HQ_ERR_UNSUPPORTED),
    "descend_then_dot": ("CIE76", 8, None, _set_then_dot, _lib.HQ_ERR_UNSUPPORTED),
    "every_negative": ("CIE76", 8, None, _set(every=-1), _lib.HQ_ERR_ARG),
    "rate_zero": ("CIE76", 8, None, _set(rate=0.0), _lib.HQ_ERR_ARG),
    "rate_nan": ("CIE76", 8, None, _set(rate=float("nan")), _lib.HQ_ERR_ARG),
    "rate_inf": ("CIE76", 8, None, _set(rate=float("inf")), _lib.HQ_ERR_ARG),
}


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_leave_the_search_alone(gpu, name):
    """Each refused call returns its status, and the run that follows is the run of a search that never
    made the call.  (A communicator of more than one rank needs two devices, more than 2^30 pixels a
    4 GiB image: both are gradient_config's lines next to the ones exercised here.)"""
    de, K, under, act, status = REFUSALS[name]
    filt = FILTERS["designed"]()
    if under == "taps":  # a bound above 2^90: no shift serves
        filt = dataclasses.replace(filt, k1=filt.k1 * np.float32(1e14))
    m = context(gpu, filt, getattr(hq.deltaETypes, de))
    try:
        rgba = noise_rgba(64, 48, 3)
        if under == "shard":
            m.setOption("shard_solo", 1)
            m.setImage(rgba.reshape(-1), None, 64, filt.illum, 16, 32)
        else:
            m.setImage(rgba.reshape(-1), None, 64, filt.illum)
        if under == "mask":
            m.setMask((np.arange(64 * 48) % 3 > 0).astype(np.uint8))
        if under == "weights":
            m.setWeights((np.arange(64 * 48) % 200 + 1).astype(np.uint8))
        never = run_search(m, K, (6,))[0]
        after, _, rc = run_search(m, K, (6,), act=act)
        assert rc == status, m._lib.hq_last_error(m.ctx)
        if name == "dot_then_descend":  # (the dot cost the case itself set stays: compare with such a search)
            never = run_search(m, K, (6,), act=lambda m, s: s.lib.hq_search_set_dot(s.h, None, 1.0))[0]
        assert after == never
    finally:
        m.close()
