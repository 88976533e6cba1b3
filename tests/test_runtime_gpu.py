"""The host runtime's housekeeping, through the C ABI: device memory comes back
after every call and every context, and a refused call leaves the context as it
was (counter-set parity, pending launch events, profiling counts)."""

import ctypes as C

import numpy as np
import pytest

import hybridquantization_amd as hq
import oracle as o
from hybridquantization_amd import _lib

pytestmark = pytest.mark.gpu
MiB = 1 << 20


@pytest.fixture(scope="module")
def hip(gpu):
    """The HIP runtime libhq has loaded, for hipMemGetInfo."""
    hq.load()
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert paths, "libhq loaded no libamdhip64"
    return C.CDLL(paths[0])


def free_bytes(hip, device):
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipSetDevice(C.c_int(device)) == 0
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def new_ctx(gpu):
    m = hq.ImageManipulation(hq.deltaETypes.CIE76, device=gpu)
    sp = hq.ScielabProcessor(72, 45.0, hq.Whitepoint.D65, None, m)
    m.illum = sp.illuminant
    return m


def small_case(seed=5):
    w = h = 64
    R, G, B = o.synthetic_image(w, h, seed=seed)
    rng = np.random.default_rng(seed)
    return o.inline_rgba(R, G, B).reshape(-1), w, rng


def palettes(rng, P, K):
    pals = rng.random((P, 4 * K), dtype=np.float32)
    pals[:, 3::4] = 0
    return pals


def test_utilities_and_contexts_give_their_memory_back(gpu, hip):
    """hq_rgb_to_xyz, hq_xyz_to_scielab, hq_quantize and hq_compute_error (with an error
    image) at n = 2^20 pixels, K = 16: after one warm-up round, 16 more rounds may not
    lower the device's free memory by more than one round's working set (the sum of the
    four calls' device buffers; a call that kept its buffers would lose 16 times that).
    Then 8 contexts, each with a 64 x 64 image and one evaluation of P = 2, K = 16,
    created and destroyed: the same bound."""
    w = h = 1024
    n, K = w * h, 16
    rng = np.random.default_rng(3)
    R, G, B = (rng.random(n, dtype=np.float32) for _ in range(3))
    rgba = o.inline_rgba(R, G, B).reshape(-1)
    colors = palettes(rng, 1, K).reshape(-1)
    f4, f1 = 16 * n, 4 * n  # a float4 buffer, a float plane
    round_bytes = ((3 * f1 + f4)  # rgb_to_xyz: R, G, B, xyz
                   + 4 * f4  # xyz_to_scielab: xyz, opponent planes, H pass, filtered planes
                   + (2 * f4 + 16 * K + 4 * K)  # quantize: in, out, colours, used flags
                   + (3 * f4 + 8 * ((n + 255) // 256)))  # compute_error: two images, error image, partial sums
    assert f4 == 16 * MiB and round_bytes > 170 * MiB
    m = new_ctx(gpu)
    try:
        def one_round():
            xyz = m.RGBtoXYZ(R, G, B)
            m.XYZtoScielab(xyz, None, None, w, m.illum)
            q = m.quantize(rgba, colors)
            img = np.zeros(4 * n, np.float32)
            m.computeError(rgba, q, img)

        one_round()
        before = free_bytes(hip, gpu)
        for _ in range(16):
            one_round()
        lost = before - free_bytes(hip, gpu)
        print(f"utilities: free memory fell by {lost / MiB:.1f} MiB over 16 rounds (bound {round_bytes / MiB:.1f})")
        assert lost <= round_bytes
    finally:
        m.close()
    img, iw, rng = small_case()
    pals = palettes(rng, 2, K)
    before = free_bytes(hip, gpu)
    for _ in range(8):
        c = new_ctx(gpu)
        c.setImage(img, None, iw, c.illum)
        assert np.all(np.isfinite(c.computeQuantizationErrorPopulation(pals, 2.0)))
        c.close()
    lost = before - free_bytes(hip, gpu)
    print(f"contexts: free memory fell by {lost / MiB:.1f} MiB over 8 contexts")
    assert lost <= round_bytes


def test_refused_evaluation_leaves_the_context_unchanged(gpu):
    """64 x 64, K = 16, profiling on: a palette-slice evaluation of a population the
    slice count does not divide (slice_ranks 2, P = 3) is HQ_ERR_ARG; with slice_ranks
    back at 1 the next evaluation gives the costs and index images of a fresh context,
    bit for bit, in exactly one assign and one cost launch."""
    img, w, rng = small_case()
    P, K = 3, 16
    pals = palettes(rng, P, K)
    lib = hq.load()

    def evaluate(m):
        costs = m.computeQuantizationErrorPopulation(pals, 2.0)
        return costs, [m.getIndices(p) for p in range(P)]

    fresh = new_ctx(gpu)
    fresh.setImage(img, None, w, fresh.illum)
    want_costs, want_idx = evaluate(fresh)
    fresh.close()

    m = new_ctx(gpu)
    try:
        m.setImage(img, None, w, m.illum)
        lib.hq_profile_enable(m.ctx, 1)
        m.setOption("slice_ranks", 2)
        part = np.full(P * (1 + K), -7.0)
        rc = lib.hq_eval_population_partial(m.ctx, _lib.fptr(pals), P, K, _lib.dptr(part))
        assert rc == _lib.HQ_ERR_ARG and np.all(part == -7.0)
        m.setOption("slice_ranks", 1)
        lib.hq_profile_reset(m.ctx)
        costs, idx = evaluate(m)
        np.testing.assert_array_equal(costs, want_costs)
        for a, b in zip(idx, want_idx):
            np.testing.assert_array_equal(a, b)
        for stage in ("assign", "cost"):
            ms, nl = C.c_double(), C.c_int64()
            _lib.check(lib.hq_profile_get(m.ctx, stage.encode(), C.byref(ms), C.byref(nl)), m.ctx)
            assert nl.value == 1 and ms.value > 0, (stage, nl.value, ms.value)
    finally:
        m.close()
