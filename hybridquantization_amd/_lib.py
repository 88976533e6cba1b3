"""ctypes binding of libhq.so (the C ABI declared in include/hq.h).

The library is built in-tree (``hybridquantization_amd/libhq.so``) by
``__graft_entry__.build()`` / ``make -C hybridquantization_amd/csrc``.  There is
no fallback: if the shared library is missing this module raises, so a GPU run
can never silently route through a CPU path.
"""

from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HQ_LIB_PATH") or os.path.join(_HERE, "libhq.so")  # override: A/B builds

HQ_OK = 0
HQ_ERR_ARG = 1
HQ_ERR_DEVICE = 2
HQ_ERR_STATE = 3
HQ_ERR_UNSUPPORTED = 4
HQ_ERR_COMM = 5
HQ_ERR_NOMEM = 6

HQ_DE_CIE76, HQ_DE_CIE94, HQ_DE_CIEDE2000 = 0, 1, 2
HQ_WP_D50, HQ_WP_D65 = 0, 1

_f = C.POINTER(C.c_float)
_d = C.POINTER(C.c_double)
_i32 = C.POINTER(C.c_int32)
_i64 = C.POINTER(C.c_int64)
_u8 = C.POINTER(C.c_uint8)
_ctx = C.c_void_p


class hq_swasa_params(C.Structure):
    _fields_ = [("population", C.c_int), ("imax", C.c_int), ("iTc", C.c_int),
                ("delta", C.c_float), ("conv_delay", C.c_float), ("conv_spread", C.c_float),
                ("t0", C.c_float), ("alpha", C.c_float), ("s0", C.c_float), ("beta", C.c_float),
                ("convergence", C.c_int)]


class hq_path_info(C.Structure):
    """include/hq.h's record of the last pass (hq_last_path); ``size`` is set by the caller."""
    _fields_ = [("size", C.c_int32), ("pass_", C.c_int32), ("sequence", C.c_int64)] + \
        [(n, C.c_int32) for n in ("ordered", "P", "K", "nch", "idx_bytes", "pixels", "grid", "argmin",
                                  "argmin_cmb", "argmin_passes", "cost", "cost_hb", "cost_de", "cost_trim",
                                  "cost_waves", "cost_nch", "cost_instance", "gen_h", "gen_h_outputs",
                                  "gen_h_split", "gen_h_rpt", "gen_v", "gen_v_rows")] + \
        [("why_not_fast", C.c_uint32), ("previous_pass", C.c_int32), ("previous_cost", C.c_int32),
         ("tiles_run", C.c_int64), ("tiles_all", C.c_int64), ("diffuse_rows", C.c_int32),
         ("diffuse_slope", C.c_int32)]


class hq_diffusion_taps(C.Structure):
    """include/hq.h's diffusion kernel: w[dy][dx + 2] / div goes from (x, y) to (x + dx, y + dy)."""
    _fields_ = [("w", (C.c_int32 * 5) * 3), ("div", C.c_int32)]


# hq.h's enum hq_diffusion, in its order
DIFFUSION_PRESETS = ("floyd_steinberg", "jarvis", "stucki", "burkes", "sierra3", "sierra2", "sierra_lite",
                     "atkinson")


class hq_dot_classes(C.Structure):
    """include/hq.h's class matrix of dot diffusion: side n, cls[y n + x] a permutation of 0 .. n n - 1."""
    _fields_ = [("n", C.c_int32), ("cls", C.c_int32 * 256)]


# hq.h's enum hq_dot_matrix, in its order
DOT_PRESETS = ("knuth8",)


# the names of hq_path_info's kinds (hq.h's enums, in their order) and of hq_path_why's bits
PATH_NAMES = {
    "pass_": ("none", "full", "assign_only", "dither"),
    "previous_pass": ("none", "full", "assign_only", "dither"),
    "previous_cost": ("none", "cost16w", "cost_mfma", "tiled_generic", "pixel_generic"),
    "pixels": ("none", "u8", "planar"),
    "grid": ("none", "build_grid", "lists16"),
    "argmin": ("none", "assign_pipe", "assign_pipe_ordered", "assign16", "assign_wide", "dither", "diffuse",
               "dot"),
    "cost": ("none", "cost16w", "cost_mfma", "tiled_generic", "pixel_generic"),
    "cost_instance": ("plain", "masked", "weighted"),
    "gen_h": ("none", "gen_hpass", "gen_hrow", "gen_hrow4", "gen_hmfma"),
    "gen_v": ("none", "gen_vpass", "gen_vtile", "gen_vtile2", "gen_vmfma"),
}
PATH_WHY = ("half", "cost_variant", "palette", "taps", "chunk_form", "nch", "wide")

EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _f, C.c_int, C.c_int, _d)
REFINE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _f, C.c_int, C.c_int)

# name -> (restype, argtypes); the exported surface of include/hq.h
SIGNATURES = {
    "hq_version": (C.c_int, []),
    "hq_status_string": (C.c_char_p, [C.c_int]),
    "hq_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "hq_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_ctx)]),
    "hq_destroy": (None, [_ctx]),
    "hq_last_error": (C.c_char_p, [_ctx]),
    "hq_design_filters": (C.c_int, [C.c_int, C.c_double, C.c_int, C.c_int, _f, _f, _f, _f,
                                    C.POINTER(C.c_int), _f]),
    "hq_set_filters": (C.c_int, [_ctx, C.c_int, _f, _f, _f, _f]),
    "hq_rgb_to_xyz": (C.c_int, [_ctx, _f, _f, _f, C.c_int64, _f]),
    "hq_xyz_to_scielab": (C.c_int, [_ctx, _f, C.c_int, C.c_int, _f, _f]),
    "hq_set_image": (C.c_int, [_ctx, _f, _f, C.c_int, C.c_int, _f]),
    "hq_set_image_shard": (C.c_int, [_ctx, _f, _f, C.c_int, C.c_int, _f, C.c_int, C.c_int]),
    "hq_set_image_planar_shard": (C.c_int, [_ctx, _f, _f, _f, C.c_int, C.c_int, _f, C.c_int,
                                            C.c_int]),
    "hq_get_labref": (C.c_int, [_ctx, _f]),
    "hq_get_image": (C.c_int, [_ctx, _f]),
    "hq_reduced_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hq_reduce_weights": (C.c_int, [_u8, C.c_int, C.c_int, C.c_int, C.c_int, _u8]),
    "hq_set_image_reduced": (C.c_int, [_ctx, _ctx, C.c_int, _f]),
    "hq_eval_population": (C.c_int, [_ctx, _f, C.c_int, C.c_int, C.c_float, _d, _i32]),
    "hq_eval_population_partial": (C.c_int, [_ctx, _f, C.c_int, C.c_int, _d]),
    "hq_get_indices": (C.c_int, [_ctx, C.c_int, _u8]),
    "hq_get_indices32": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_uint32)]),
    "hq_get_pixel_errors": (C.c_int, [_ctx, C.c_int, _f]),
    "hq_cluster_sums": (C.c_int, [_ctx, C.c_int, C.c_int, _i64, _i64]),
    "hq_centroids_from_sums": (C.c_int, [_i64, C.c_int64, C.c_int, C.c_int, _f]),
    "hq_refine_population": (C.c_int, [_ctx, _f, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _d,
                                       _i32, _d]),
    "hq_cluster_errors": (C.c_int, [_ctx, C.c_int, C.c_int, _i64, _f]),
    "hq_reseed_unused": (C.c_int, [_i64, _f, C.c_int, C.c_int, C.c_int, _f, C.POINTER(C.c_int)]),
    "hq_reseed_unused_fixed": (C.c_int, [_i64, _f, C.c_int, C.c_int, C.c_int, C.c_int, _f, C.POINTER(C.c_int)]),
    "hq_set_fixed_colors": (C.c_int, [_ctx, _f, C.c_int]),
    "hq_fixed_colors": (C.c_int, [_ctx, C.POINTER(C.c_int), _f]),
    "hq_swasa_search_host_fixed": (C.c_int, [C.POINTER(hq_swasa_params), C.c_int, C.c_uint64, C.c_int, EVAL_FN,
                                             REFINE_FN, C.c_int, _f, _f, C.c_int, C.c_void_p, _f, _d, _d]),
    "hq_repair_population": (C.c_int, [_ctx, _f, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                       _d, _i32, _d]),
    "hq_dither_population": (C.c_int, [_ctx, _f, C.c_int, C.c_int, C.c_float, C.c_float, _d, _i32]),
    "hq_diffusion_preset": (C.c_int, [C.c_int, C.POINTER(hq_diffusion_taps)]),
    "hq_diffusion_taps_legal": (C.c_int, [C.POINTER(hq_diffusion_taps)]),
    "hq_diffusion_classify": (C.c_int, [C.POINTER(hq_diffusion_taps), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hq_diffuse_population": (C.c_int, [_ctx, _f, C.c_int, C.c_int, C.POINTER(hq_diffusion_taps), C.c_float,
                                        C.c_float, _d, _i32]),
    "hq_dot_preset": (C.c_int, [C.c_int, C.POINTER(hq_dot_classes)]),
    "hq_dot_classes_legal": (C.c_int, [C.POINTER(hq_dot_classes)]),
    "hq_dot_barons": (C.c_int, [C.POINTER(hq_dot_classes)]),
    "hq_dot_population": (C.c_int, [_ctx, _f, C.c_int, C.c_int, C.POINTER(hq_dot_classes), C.c_float, C.c_float,
                                    _d, _i32]),
    "hq_dot_reach": (C.c_int, [C.POINTER(hq_dot_classes), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hq_dot_apron": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hq_dot_reach2": (C.c_int, [C.POINTER(hq_dot_classes)] + [C.POINTER(C.c_int)] * 4),
    "hq_dot_levels": (C.c_int, [C.POINTER(hq_dot_classes), _i32, C.POINTER(C.c_int)]),
    "hq_dot_form": (C.c_int, [_ctx] + [C.POINTER(C.c_int)] * 4),
    "hq_dot_population_partial": (C.c_int, [_ctx, _f, C.c_int, C.c_int, C.POINTER(hq_dot_classes), C.c_float, _d]),
    "hq_bayer_map": (C.c_int, [C.c_int, _f]),
    "hq_set_dither_map": (C.c_int, [_ctx, _f, C.c_int, C.c_int]),
    "hq_ordered_population": (C.c_int, [_ctx, _f, C.c_int, C.c_int, _f, C.c_float, _d, _i32]),
    "hq_ordered_population_partial": (C.c_int, [_ctx, _f, C.c_int, C.c_int, _f, _d]),
    "hq_set_mask": (C.c_int, [_ctx, _u8, C.c_int, C.c_int]),
    "hq_mask_info": (C.c_int, [_ctx, _i64, _i64, _i64, _i64]),
    "hq_set_weights": (C.c_int, [_ctx, _u8, C.c_int, C.c_int]),
    "hq_weights_info": (C.c_int, [_ctx, _i64, _i64]),
    "hq_color_histogram": (C.c_int, [_ctx, C.c_int, _i64, _i64]),
    "hq_median_cut": (C.c_int, [_i64, C.c_int, C.c_int64, C.c_int, _f, C.POINTER(C.c_int)]),
    "hq_quantize": (C.c_int, [_ctx, _f, C.c_int64, _f, C.c_int, _f, _i32]),
    "hq_assign_coords": (C.c_int, [_ctx, C.c_int, _f, C.c_int64, _f]),
    "hq_compute_error": (C.c_int, [_ctx, _f, _f, C.c_int64, _f, _d]),
    "hq_comm_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "hq_comm_init": (C.c_int, [_ctx, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]),
    "hq_comm_info": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hq_swasa_default_params": (None, [C.POINTER(hq_swasa_params)]),
    "hq_search_create": (C.c_int, [_ctx, C.POINTER(hq_swasa_params), C.c_int, C.c_uint64,
                                   C.POINTER(C.c_void_p)]),
    "hq_search_create_from": (C.c_int, [_ctx, C.POINTER(hq_swasa_params), C.c_int, C.c_uint64, _f,
                                        C.POINTER(C.c_void_p)]),
    "hq_search_run": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "hq_search_best": (C.c_int, [C.c_void_p, _f, _d, C.POINTER(C.c_int)]),
    "hq_search_population": (C.c_int, [C.c_void_p, _f, _d]),
    "hq_search_destroy": (None, [C.c_void_p]),
    "hq_search_set_lloyd": (C.c_int, [C.c_void_p, C.c_int]),
    "hq_search_set_repair": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hq_search_set_ordered": (C.c_int, [C.c_void_p, _f]),
    "hq_search_set_dot": (C.c_int, [C.c_void_p, C.POINTER(hq_dot_classes), C.c_float]),
    "hq_swasa_search_host": (C.c_int, [C.POINTER(hq_swasa_params), C.c_int, C.c_uint64,
                                       C.c_int, EVAL_FN, C.c_void_p, _f, _d, _d]),
    "hq_swasa_search_host_lloyd": (C.c_int, [C.POINTER(hq_swasa_params), C.c_int, C.c_uint64,
                                             C.c_int, EVAL_FN, REFINE_FN, C.c_int, C.c_void_p, _f, _d, _d]),
    "hq_swasa_search_host_from": (C.c_int, [C.POINTER(hq_swasa_params), C.c_int, C.c_uint64,
                                            C.c_int, EVAL_FN, REFINE_FN, C.c_int, _f, C.c_void_p, _f, _d, _d]),
    "hq_profile_enable": (C.c_int, [_ctx, C.c_int]),
    "hq_profile_get": (C.c_int, [_ctx, C.c_char_p, _d, C.POINTER(C.c_int64)]),
    "hq_profile_reset": (C.c_int, [_ctx]),
    "hq_last_path": (C.c_int, [_ctx, C.POINTER(hq_path_info)]),
    "hq_search_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hq_set_option": (C.c_int, [_ctx, C.c_char_p, C.c_int]),
}

_LIB = None


class HQError(RuntimeError):
    def __init__(self, status: int, msg: str = ""):
        self.status = status
        super().__init__(f"libhq status {status}: {msg}")


class HQUnavailable(HQError):
    """No usable GPU / library: the reference's IM:79-92 fallback condition."""


def load():
    """Load libhq.so (raises OSError if it has not been built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} not found: build it with __graft_entry__.build() "
                          "(make -C hybridquantization_amd/csrc); there is no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def check(status: int, ctx=None):
    if status != HQ_OK:
        lib = load()
        msg = lib.hq_last_error(ctx).decode() if ctx else lib.hq_status_string(status).decode()
        if status == HQ_ERR_DEVICE:
            raise HQUnavailable(status, msg)
        raise HQError(status, msg)


def fptr(a):
    return a.ctypes.data_as(_f)


def dptr(a):
    return a.ctypes.data_as(_d)


def iptr(a):
    return a.ctypes.data_as(_i32)


def i64ptr(a):
    return a.ctypes.data_as(_i64)


def u8ptr(a):
    return a.ctypes.data_as(_u8)
