"""ctypes binding of include/rt_api.h (one Python method per C entry point)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

SPHERE_DT = np.dtype([("rad", "<f4"), ("p", "<f4", 3), ("e", "<f4", 3), ("c", "<f4", 3),
                      ("refl", "<i4")])           # include/rt_api.h rt_sphere, 44 bytes
CAMERA_FLOATS = 15                                # rt_camera: orig,target,dir,x,y

RT_MODE_PARITY, RT_MODE_FAST = 0, 1
DIFF, SPEC, REFR = 0, 1, 2

# every symbol include/rt_api.h declares = the export table of librt_hip.so (tests/test_abi.py)
SYMBOLS = ["rt_render", "rt_release_cache", "rt_create", "rt_create_multi", "rt_create_multi_on", "rt_shard_count", "rt_last_kernel", "rt_scene_choice",
           "rt_create_sharded", "rt_destroy", "rt_set_scene", "rt_update_spheres_async",
           "rt_set_camera", "rt_set_mode", "rt_reset", "rt_reset_async", "rt_render_pass", "rt_render_async",
           "rt_pin_output", "rt_set_pixel_write", "rt_read_pixels", "rt_read_pixels_async", "rt_throttle", "rt_device_pixels", "rt_set_pixel_buffer", "rt_stream",
           "rt_local_rows", "rt_current_sample", "rt_read_colors",
           "rt_read_seeds", "rt_get_stats", "rt_last_error", "rt_deinterleave_rows", "rt_compute_camera",
           "rt_default_seeds", "rt_demo_scene", "rt_read_scene", "rt_build_id",
           "rt_stream_seeds", "rt_seed_stream_async", "rt_write_state", "rt_save_state", "rt_load_state", "rt_merge_async",
           "rt_compare_tiles", "rt_compare_async", "rt_compare", "rt_error_psnr", "rt_render_converged",
           "rt_tile_passes", "rt_select_tiles", "rt_render_tiles_async", "rt_render_adaptive",
           "rt_denoise_defaults", "rt_denoise_async", "rt_denoise_planes",
           "rt_denoise_pair_async", "rt_denoise_pair_planes", "rt_read_filtered", "rt_compare_filtered_async", "rt_compare_filtered",
           "rt_render_converged_filtered", "rt_render_adaptive_filtered", "rt_denoise_pair_tiles_async", "rt_render_adaptive_filtered_tiles",
           "rt_guide_defaults", "rt_features_async", "rt_last_features_kernel", "rt_read_features", "rt_features_planes", "rt_set_denoise_guide",
           "rt_denoise_guided_planes", "rt_denoise_pair_guided_planes",
           "rt_reproject_defaults", "rt_reproject_async", "rt_read_temporal", "rt_reproject_planes",
           "rt_atrous_defaults", "rt_atrous_async", "rt_read_atrous", "rt_atrous_planes",
           "rt_moments_defaults", "rt_set_temporal_moments", "rt_read_moments", "rt_reproject_moments_planes", "rt_atrous_moments_planes",
           "rt_shadow_history_defaults", "rt_set_shadow_history", "rt_read_history_flags", "rt_reproject_shadow_planes", "rt_shadow_history_pairs"]
# include/rt_debug.h: what librt_hip_diag.so exports on top of that
DEBUG_SYMBOLS = ["rt_debug_variant_count", "rt_debug_instance", "rt_debug_instance_name", "rt_debug_shard_kernel", "rt_debug_break_gather", "rt_debug_set_rccl_library", "rt_debug_stage_tables", "rt_debug_eval", "rt_debug_sqrt_mismatches", "rt_debug_hitpost_mismatches",
                 "rt_debug_rcp_probe", "rt_debug_set_regen_gate", "rt_debug_set_mat_lds_limit", "rt_debug_set_persist",
                 "rt_debug_set_ncus", "rt_debug_set_coop_min", "rt_debug_set_bvh", "rt_debug_set_tree_shape", "rt_debug_set_bvh_layout", "rt_debug_set_walk", "rt_debug_set_walk_round", "rt_debug_bvh_pick", "rt_debug_tree_estimate", "rt_debug_set_choice_estimate", "rt_debug_create_breakdown", "rt_debug_walk_rays", "rt_debug_read_bvh", "rt_debug_read_packed_pairs", "rt_debug_set_direct_camera", "rt_debug_tile_candidates", "rt_debug_set_tile_order", "rt_debug_read_tile_order", "rt_debug_read_tile_list", "rt_debug_set_wg_waves", "rt_debug_counters", "rt_debug_counters_raw",
                 "rt_debug_reset_by_copy", "rt_debug_probe_seeds", "rt_debug_sidelog_read", "rt_debug_timelog_enable", "rt_debug_timelog_tag",
                 "rt_debug_timelog_read", "rt_debug_wavelog_read", "rt_debug_set_features_form"]


class RtError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"rt status {code}: {text}")
        self.code = code


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("rng_draws", C.c_uint64), ("launches", C.c_uint64),
                ("last_kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FrameError(C.Structure):
    """include/rt_api.h rt_frame_error (48 bytes): exact integer sums over the 8-bit channels of two packed frames."""
    _fields_ = [("sq_err", C.c_uint64 * 3), ("differing", C.c_uint64), ("pixels", C.c_uint64), ("max_abs", C.c_uint32),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        return {"sq_err": [int(v) for v in self.sq_err], "differing": int(self.differing), "pixels": int(self.pixels),
                "max_abs": int(self.max_abs), "reserved": int(self.reserved)}

    @classmethod
    def from_dict(cls, d):
        return cls((C.c_uint64 * 3)(*d["sq_err"]), d["differing"], d["pixels"], d["max_abs"], d.get("reserved", 0))


class DenoiseParams(C.Structure):
    """include/rt_api.h rt_denoise_params (16 bytes): search radius R, patch radius P, alpha, k."""
    _fields_ = [("search_radius", C.c_int32), ("patch_radius", C.c_int32), ("alpha", C.c_float), ("k", C.c_float)]

    def as_dict(self):
        return {"search_radius": int(self.search_radius), "patch_radius": int(self.patch_radius), "alpha": float(self.alpha), "k": float(self.k)}


class GuideParams(C.Structure):
    """include/rt_api.h rt_guide_params (16 bytes): k_albedo, k_normal, k_depth, reserved (0)."""
    _fields_ = [("k_albedo", C.c_float), ("k_normal", C.c_float), ("k_depth", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {"k_albedo": float(self.k_albedo), "k_normal": float(self.k_normal), "k_depth": float(self.k_depth), "reserved": int(self.reserved)}


class ReprojectParams(C.Structure):
    """include/rt_api.h rt_reproject_params (16 bytes): k_pos, max_history, two reserved words (0)."""
    _fields_ = [("k_pos", C.c_float), ("max_history", C.c_float), ("reserved", C.c_uint32 * 2)]

    def as_dict(self):
        return {"k_pos": float(self.k_pos), "max_history": float(self.max_history), "reserved": [int(v) for v in self.reserved]}


class ReprojectView(C.Structure):
    """include/rt_api.h rt_reproject_view: one side of rt_reproject_planes."""
    _fields_ = [("plane", C.c_void_p), ("channels", C.c_int), ("passes", C.c_int), ("feat", C.c_void_p), ("cam", C.c_void_p), ("spheres", C.c_void_p)]


class AtrousParams(C.Structure):
    """include/rt_api.h rt_atrous_params (16 bytes): levels (0 .. 5), k_lum, k_normal, a reserved word (0)."""
    _fields_ = [("levels", C.c_int32), ("k_lum", C.c_float), ("k_normal", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {"levels": int(self.levels), "k_lum": float(self.k_lum), "k_normal": float(self.k_normal), "reserved": int(self.reserved)}


class MomentsParams(C.Structure):
    """include/rt_api.h rt_moments_params (16 bytes): k_min (finite, >= 1), three reserved words (0)."""
    _fields_ = [("k_min", C.c_float), ("reserved", C.c_uint32 * 3)]

    def as_dict(self):
        return {"k_min": float(self.k_min), "reserved": [int(v) for v in self.reserved]}


class ShadowHistoryParams(C.Structure):
    """include/rt_api.h rt_shadow_history_params (16 bytes): keep (finite, >= 0), three reserved words (0)."""
    _fields_ = [("keep", C.c_float), ("reserved", C.c_uint32 * 3)]

    def as_dict(self):
        return {"keep": float(self.keep), "reserved": [int(v) for v in self.reserved]}


SHADOW_PAIR_CHUNK = 64      # include/rt_api.h RT_SHADOW_PAIR_CHUNK: the pairs of rule 29 the kernels stage in LDS at a time


class _Scene(C.Structure):
    _fields_ = [("spheres", C.c_void_p), ("count", C.c_uint32)]


def lib_path(diag=False):
    return os.path.join(_HERE, "librt_hip_diag.so" if diag else "librt_hip.so")


_libs = {}


def load_library(diag=False):
    """Load librt_hip.so (built in-tree by raytracing_simple_amd._build).  Raises if absent:
    the HIP library IS the product, there is nothing to fall back to.  diag=True loads the
    diagnostics build instead (librt_hip_diag.so: include/rt_debug.h on top of the same ABI; tests and
    tools only -- bench.py and the product paths never do)."""
    if diag in _libs:
        return _libs[diag]
    path = lib_path(diag)
    if not os.path.exists(path):
        raise RtError(-2, f"{path} is not built; run `python -m raytracing_simple_amd._build` "
                          "(needs hipcc) -- there is no CPU fallback")
    lib = C.CDLL(path)
    vp, i32, u32, sz = C.c_void_p, C.c_int, C.c_uint32, C.c_size_t
    u64p = C.POINTER(C.c_ulonglong)
    sig = {
        "rt_render": (i32, [vp, vp, vp, i32, i32, i32]),
        "rt_release_cache": (None, []),
        "rt_create_multi": (i32, [C.POINTER(vp), i32, i32, i32]),
        "rt_create_multi_on": (i32, [C.POINTER(vp), i32, i32, C.POINTER(i32), i32, i32]),
        "rt_shard_count": (i32, [vp]),
        "rt_last_kernel": (C.c_char_p, [vp]),
        "rt_scene_choice": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "rt_build_id": (C.c_char_p, []),
        "rt_update_spheres_async": (i32, [vp, u32, u32, vp, vp]),
        "rt_read_pixels": (i32, [vp, vp]),
        "rt_read_pixels_async": (i32, [vp, vp, vp]),
        "rt_throttle": (i32, [vp, i32, C.POINTER(C.c_double)]),
        "rt_deinterleave_rows": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        "rt_create": (i32, [C.POINTER(vp), i32, i32]),
        "rt_create_sharded": (i32, [C.POINTER(vp), i32, i32, i32, i32, i32, i32]),
        "rt_destroy": (None, [vp]),
        "rt_set_scene": (i32, [vp, vp, u32]),
        "rt_set_camera": (i32, [vp, vp]),
        "rt_set_mode": (i32, [vp, i32]),
        "rt_reset": (i32, [vp]),
        "rt_reset_async": (i32, [vp, vp]),
        "rt_render_pass": (i32, [vp, vp, i32]),
        "rt_render_async": (i32, [vp, i32, vp]),
        "rt_device_pixels": (i32, [vp, C.POINTER(vp), C.POINTER(sz)]),
        "rt_set_pixel_buffer": (i32, [vp, vp, sz]),
        "rt_pin_output": (i32, [vp, vp, sz]),
        "rt_set_pixel_write": (i32, [vp, i32]),
        "rt_stream": (vp, [vp]),
        "rt_local_rows": (i32, [vp]),
        "rt_current_sample": (i32, [vp]),
        "rt_read_colors": (i32, [vp, vp]),
        "rt_read_seeds": (i32, [vp, vp]),
        "rt_get_stats": (i32, [vp, C.POINTER(Stats)]),
        "rt_last_error": (C.c_char_p, []),
        "rt_compute_camera": (None, [vp, i32, i32]),
        "rt_default_seeds": (None, [vp, sz]),
        "rt_stream_seeds": (None, [C.c_uint64, vp, sz]),
        "rt_seed_stream_async": (i32, [vp, C.c_uint64, vp]),
        "rt_write_state": (i32, [vp, vp, vp, i32]),
        "rt_save_state": (i32, [vp, C.c_char_p]),
        "rt_load_state": (i32, [vp, C.c_char_p]),
        "rt_merge_async": (i32, [vp, C.POINTER(vp), i32, vp]),
        "rt_compare_tiles": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "rt_compare_async": (i32, [vp, vp, vp, vp, vp]),
        "rt_compare": (i32, [vp, vp, C.POINTER(FrameError), vp]),
        "rt_error_psnr": (C.c_double, [C.POINTER(FrameError)]),
        "rt_render_converged": (i32, [vp, vp, C.c_double, i32, i32, C.POINTER(FrameError), C.POINTER(i32)]),
        "rt_tile_passes": (i32, [vp, vp]),
        "rt_select_tiles": (i32, [vp, vp, u32, vp, C.POINTER(u32)]),
        "rt_render_tiles_async": (i32, [vp, i32, vp]),
        "rt_render_adaptive": (i32, [vp, vp, C.c_double, i32, i32, i32, C.POINTER(FrameError), C.POINTER(i32)]),
        "rt_denoise_defaults": (None, [C.POINTER(DenoiseParams)]),
        "rt_denoise_async": (i32, [vp, vp, vp, C.POINTER(DenoiseParams), vp]),
        "rt_denoise_planes": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(DenoiseParams)]),
        "rt_denoise_pair_async": (i32, [vp, vp, C.POINTER(DenoiseParams), vp]),
        "rt_denoise_pair_planes": (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(DenoiseParams)]),
        "rt_read_filtered": (i32, [vp, vp]),
        "rt_compare_filtered_async": (i32, [vp, vp, vp, vp, vp]),
        "rt_compare_filtered": (i32, [vp, vp, C.POINTER(FrameError), vp]),
        "rt_render_converged_filtered": (i32, [vp, vp, C.c_double, i32, i32, C.POINTER(DenoiseParams), C.POINTER(FrameError), C.POINTER(i32)]),
        "rt_render_adaptive_filtered": (i32, [vp, vp, C.c_double, i32, i32, i32, C.POINTER(DenoiseParams), C.POINTER(FrameError), C.POINTER(i32)]),
        "rt_denoise_pair_tiles_async": (i32, [vp, vp, C.POINTER(DenoiseParams), vp]),
        "rt_render_adaptive_filtered_tiles": (i32, [vp, vp, C.c_double, i32, i32, i32, C.POINTER(DenoiseParams), C.POINTER(FrameError), C.POINTER(i32)]),
        "rt_guide_defaults": (None, [C.POINTER(GuideParams)]),
        "rt_features_async": (i32, [vp, vp]),
        "rt_last_features_kernel": (C.c_char_p, [vp]),
        "rt_read_features": (i32, [vp, vp]),
        "rt_features_planes": (i32, [vp, vp, u32, vp, i32, i32]),
        "rt_set_denoise_guide": (i32, [vp, C.POINTER(GuideParams)]),
        "rt_denoise_guided_planes": (i32, [vp, vp, vp, vp, vp, i32, i32, C.POINTER(DenoiseParams), C.POINTER(GuideParams)]),
        "rt_denoise_pair_guided_planes": (i32, [vp, vp, vp, vp, vp, i32, i32, C.POINTER(DenoiseParams), C.POINTER(GuideParams)]),
        "rt_reproject_defaults": (None, [C.POINTER(ReprojectParams)]),
        "rt_reproject_async": (i32, [vp, vp, C.POINTER(ReprojectParams), vp]),
        "rt_read_temporal": (i32, [vp, vp, vp]),
        "rt_reproject_planes": (i32, [vp, C.POINTER(ReprojectView), C.POINTER(ReprojectView), u32, i32, i32, C.POINTER(ReprojectParams)]),
        "rt_atrous_defaults": (None, [C.POINTER(AtrousParams)]),
        "rt_atrous_async": (i32, [vp, C.POINTER(AtrousParams), vp]),
        "rt_read_atrous": (i32, [vp, vp, vp]),
        "rt_atrous_planes": (i32, [vp, vp, i32, i32, vp, i32, i32, C.POINTER(AtrousParams)]),
        "rt_moments_defaults": (None, [C.POINTER(MomentsParams)]),
        "rt_set_temporal_moments": (i32, [vp, C.POINTER(MomentsParams)]),
        "rt_read_moments": (i32, [vp, vp]),
        "rt_reproject_moments_planes": (i32, [vp, vp, C.POINTER(ReprojectView), C.POINTER(ReprojectView), vp, u32, i32, i32, C.POINTER(ReprojectParams)]),
        "rt_atrous_moments_planes": (i32, [vp, vp, i32, i32, vp, vp, i32, i32, C.POINTER(AtrousParams), C.POINTER(MomentsParams)]),
        "rt_shadow_history_defaults": (None, [C.POINTER(ShadowHistoryParams)]),
        "rt_set_shadow_history": (i32, [vp, C.POINTER(ShadowHistoryParams)]),
        "rt_read_history_flags": (i32, [vp, vp]),
        "rt_reproject_shadow_planes": (i32, [vp, vp, vp, C.POINTER(ReprojectView), C.POINTER(ReprojectView), vp, u32, i32, i32, C.POINTER(ReprojectParams),
                                             C.POINTER(ShadowHistoryParams)]),
        "rt_shadow_history_pairs": (i32, [vp, vp, u32, vp, u32]),
        "rt_demo_scene": (i32, [vp, u32]),
        "rt_read_scene": (i32, [C.c_char_p, vp, u32, C.POINTER(u32), vp, vp, i32]),
    }
    if diag:
        sig.update({
            "rt_debug_variant_count": (i32, [i32]),
            "rt_debug_instance": (i32, [C.c_char_p]),
            "rt_debug_instance_name": (C.c_char_p, [i32, i32]),
            "rt_debug_shard_kernel": (C.c_char_p, [vp, i32]),
            "rt_debug_break_gather": (i32, [vp]),
            "rt_debug_set_rccl_library": (i32, [C.c_char_p, i32]),
            "rt_debug_stage_tables": (i32, [vp, i32, i32]),
            "rt_debug_eval": (i32, [i32, vp, vp, sz]),
            "rt_debug_sqrt_mismatches": (C.c_longlong, []),
            "rt_debug_hitpost_mismatches": (C.c_longlong, []),
            "rt_debug_rcp_probe": (i32, [vp]),
            "rt_debug_set_regen_gate": (i32, [vp, i32]),
            "rt_debug_set_mat_lds_limit": (i32, [vp, i32]),
            "rt_debug_set_persist": (i32, [vp, i32]),
            "rt_debug_set_ncus": (i32, [vp, i32]),
            "rt_debug_set_direct_camera": (i32, [vp, i32]),
            "rt_debug_tile_candidates": (i32, [vp, i32, i32, vp, u32, i32, i32, i32, vp]),
            "rt_debug_set_coop_min": (i32, [vp, i32]),
            "rt_debug_set_bvh": (i32, [vp, i32, i32]),
            "rt_debug_set_tree_shape": (i32, [vp, i32]),
            "rt_debug_set_bvh_layout": (i32, [vp, i32, i32]),
            "rt_debug_set_walk": (i32, [vp, i32, i32, i32]),
            "rt_debug_bvh_pick": (i32, [vp]),
            "rt_debug_tree_estimate": (i32, [vp, C.POINTER(C.c_double)]),
            "rt_debug_set_choice_estimate": (i32, [vp, i32]),
            "rt_debug_create_breakdown": (i32, [C.POINTER(C.c_double)]),
            "rt_debug_walk_rays": (i32, [vp, vp, u32, vp]),
            "rt_debug_set_walk_round": (i32, [vp, i32]),
            "rt_debug_set_features_form": (i32, [vp, i32]),
            "rt_debug_read_bvh": (i32, [vp, vp, u32, vp]),
            "rt_debug_read_packed_pairs": (i32, [vp, vp, u32, C.POINTER(u32)]),
            "rt_debug_set_tile_order": (i32, [vp, i32]),
            "rt_debug_set_wg_waves": (i32, [vp, i32]),
            "rt_debug_read_tile_order": (i32, [vp, vp, vp, u32, C.POINTER(u32), C.POINTER(i32)]),
            "rt_debug_read_tile_list": (i32, [vp, vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(i32)]),
            "rt_debug_counters": (i32, [vp, vp]),
            "rt_debug_counters_raw": (i32, [vp, vp]),
            "rt_debug_reset_by_copy": (i32, [vp, vp, i32]),
            "rt_debug_probe_seeds": (i32, [vp, vp, i32]),
            "rt_debug_sidelog_read": (i32, [vp, u32, vp, vp]),
            "rt_debug_timelog_enable": (i32, [vp, u32, u32]),
            "rt_debug_timelog_tag": (i32, [vp, C.c_ulonglong]),
            "rt_debug_timelog_read": (i32, [vp, vp, u32, C.POINTER(u32)]),
            "rt_debug_wavelog_read": (i32, [vp, vp, u32]),
        })
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _libs[diag] = lib
    return lib


def _check(rc, lib=None):
    if rc != 0:
        raise RtError(rc, (lib or load_library()).rt_last_error().decode(errors="replace"))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def as_spheres(spheres):
    """Sphere records as the 44-byte structured dtype; raw bytes (uint8, a multiple of 44) are
    reinterpreted, anything else is refused rather than silently given another sphere count."""
    a = np.ascontiguousarray(spheres)
    if a.dtype != SPHERE_DT:
        if a.dtype != np.uint8 or a.size % SPHERE_DT.itemsize:
            raise TypeError(f"spheres must be SPHERE_DT records or their raw bytes, not {a.dtype}[{a.size}]")
        a = a.reshape(-1).view(SPHERE_DT)
    return a


def as_camera(cam):
    a = np.ascontiguousarray(cam, dtype=np.float32).reshape(-1)
    if a.size != CAMERA_FLOATS:
        raise ValueError("camera = 15 floats: orig, target, dir, x, y")
    return a


def render(spheres, cam, w, h, spp):
    """rt_render: the one-shot headline call.  Returns uint32[h*w] (row 0 = bottom)."""
    lib = load_library()
    sph = as_spheres(spheres)
    cam = as_camera(cam)
    out = np.zeros(w * h, np.uint32)
    scene = _Scene(sph.ctypes.data, len(sph))
    _check(lib.rt_render(C.addressof(scene), _ptr(cam), _ptr(out), w, h, spp))
    return out


class RtContext:
    """One rt_ctx (= one OpenCLConfigBuffer of the reference).

    devices=[...] makes it a multi-device context (rt_create_multi_on): the image sharded over those
    HIP devices of this process, one RCCL gather per frame (a device listed twice = the one-GPU
    rehearsal of that path).  diag=True binds the diagnostics library (tests / tools only)."""

    def __init__(self, w, h, device=0, rank=0, nranks=1, tile_rows=8, devices=None, diag=False):
        self._lib = load_library(diag)
        self._h = C.c_void_p()
        self.w, self.h = w, h
        self.rank, self.nranks, self.tile_rows = rank, nranks, tile_rows
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            self._check(self._lib.rt_create_multi_on(C.byref(self._h), w, h, arr, len(devices), tile_rows))
            self.rank, self.nranks = 0, 1           # the front of a multi-device context is the whole image
        else:
            self._check(self._lib.rt_create_sharded(C.byref(self._h), w, h, device, rank, nranks, tile_rows))

    def _check(self, rc):
        _check(rc, self._lib)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown: modules may already be gone
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # --- state ---------------------------------------------------------------------------
    def set_scene(self, spheres):
        sph = as_spheres(spheres)
        self._check(self._lib.rt_set_scene(self._h, _ptr(sph), len(sph)))

    def set_camera(self, cam):
        cam = as_camera(cam)
        self._check(self._lib.rt_set_camera(self._h, _ptr(cam)))

    def set_mode(self, mode):
        self._check(self._lib.rt_set_mode(self._h, mode))

    def reset(self):
        self._check(self._lib.rt_reset(self._h))

    @property
    def local_rows(self):
        return self._lib.rt_local_rows(self._h)

    @property
    def current_sample(self):
        return self._lib.rt_current_sample(self._h)

    # --- rendering ----------------------------------------------------------------------
    def render_pass(self, n_samples, copy=True, out=None):
        """n_samples reference passes in one launch; returns the local pixel rows (uint32),
        written into `out` when one is given (a C-contiguous uint32 array of that size)."""
        if out is None:
            out = np.zeros(self.local_rows * self.w, np.uint32) if copy else None
        elif out.dtype != np.uint32 or out.size < self.local_rows * self.w or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous uint32 array of local_rows * w elements")
        self._check(self._lib.rt_render_pass(self._h, _ptr(out) if out is not None else None, n_samples))
        return out

    def set_pixel_write(self, enable):
        self._check(self._lib.rt_set_pixel_write(self._h, 1 if enable else 0))

    def pin_output(self, out):
        """Page-lock `out` (the array later passed to render_pass(out=...)) for full-rate readback;
        None unpins.  The array must outlive the pin."""
        if out is None:
            self._check(self._lib.rt_pin_output(self._h, None, 0))
        else:
            self._check(self._lib.rt_pin_output(self._h, _ptr(out), out.size))

    def read_pixels(self):
        """rt_read_pixels: the up-to-date packed frame (packs it from the running average first if the
        last launches ran with the pixel store off)."""
        out = np.zeros(self.local_rows * self.w, np.uint32)
        self._check(self._lib.rt_read_pixels(self._h, _ptr(out)))
        return out

    def read_pixels_async(self, out, stream=None):
        """rt_read_pixels_async: queue the copy of the up-to-date frame into `out` (page-lock it with pin_output)."""
        self._check(self._lib.rt_read_pixels_async(self._h, _ptr(out), C.c_void_p(stream or 0)))

    def throttle(self, max_in_flight):
        """rt_throttle: wait until at most `max_in_flight` render_async launches are unfinished; returns the device
        time per pass (ms) of the most recent finished one (0.0 if none)."""
        ms = C.c_double()
        self._check(self._lib.rt_throttle(self._h, max_in_flight, C.byref(ms)))
        return ms.value

    def update_spheres(self, first, spheres, stream=None):
        """rt_update_spheres_async: replace spheres [first, first+len) of the current scene."""
        sph = as_spheres(spheres)
        self._check(self._lib.rt_update_spheres_async(self._h, first, len(sph), _ptr(sph), C.c_void_p(stream or 0)))

    @property
    def last_kernel(self):
        """Symbol of the kernel instance the last launch used (rt_last_kernel)."""
        return self._lib.rt_last_kernel(self._h).decode()

    def scene_choice(self):
        """rt_scene_choice: {'picked': 0 | 'hierarchy' | 'sweep', and the two measured ms per pass}."""
        a, b = C.c_double(), C.c_double()
        k = self._lib.rt_scene_choice(self._h, C.byref(a), C.byref(b))
        return {"picked": {0: None, 1: "hierarchy", 2: "sweep"}.get(k), "hierarchy_ms_per_pass": a.value, "sweep_ms_per_pass": b.value}

    @property
    def shard_count(self):
        return self._lib.rt_shard_count(self._h)

    def reset_async(self, stream=None):
        self._check(self._lib.rt_reset_async(self._h, C.c_void_p(stream or 0)))

    def render_async(self, n_samples, stream=None):
        self._check(self._lib.rt_render_async(self._h, n_samples, C.c_void_p(stream or 0)))

    def set_pixel_buffer(self, dptr, count):
        """Later launches write their packed pixels to this device address (None = own buffer)."""
        self._check(self._lib.rt_set_pixel_buffer(self._h, C.c_void_p(dptr or 0), count))

    @property
    def stream(self):
        """Raw hipStream_t of the context's own stream (wrap with torch.cuda.ExternalStream)."""
        return self._lib.rt_stream(self._h)

    def device_pixels(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._lib.rt_device_pixels(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def device_pixels_array(self):
        """The local pixel rows as a zero-copy __cuda_array_interface__ object (int32 [rows, w]),
        for torch.as_tensor(..., device='cuda') in the multi-GPU gather."""
        ptr, n = self.device_pixels()

        class _View:
            pass

        v = _View()
        v.__cuda_array_interface__ = {"shape": (n // self.w, self.w), "typestr": "<i4",
                                      "data": (ptr, False), "version": 2, "strides": None}
        v._owner = self
        return v

    def read_colors(self):
        out = np.zeros(3 * self.w * self.h, np.float32)
        self._check(self._lib.rt_read_colors(self._h, _ptr(out)))
        return out

    def read_seeds(self):
        out = np.zeros(2 * self.w * self.h, np.uint32)
        self._check(self._lib.rt_read_seeds(self._h, _ptr(out)))
        return out

    # --- render state in and out (rt_state.hip) -------------------------------------------
    def seed_stream(self, stream_id, stream=None):
        """rt_seed_stream_async: pass 0 of seed stream `stream_id` (0 = the default stream), seeded on the device."""
        self._check(self._lib.rt_seed_stream_async(self._h, stream_id, C.c_void_p(stream or 0)))

    def write_state(self, colors, seeds, current_sample):
        """rt_write_state: colour plane and seeds as read_colors() / read_seeds() return them (None: the default stream;
        colours may be None only at pass 0), and the pass number the next launch continues from."""
        def arr(a, dt, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
            if a.size != n:
                raise ValueError("expected %d elements, got %d" % (n, a.size))
            return a
        col, sd = arr(colors, np.float32, 3 * self.w * self.h), arr(seeds, np.uint32, 2 * self.w * self.h)
        self._check(self._lib.rt_write_state(self._h, _ptr(col) if col is not None else None, _ptr(sd) if sd is not None else None,
                                             current_sample))

    def save_state(self, path):
        self._check(self._lib.rt_save_state(self._h, os.fsencode(path)))

    def load_state(self, path):
        self._check(self._lib.rt_load_state(self._h, os.fsencode(path)))

    def merge(self, sources, stream=None):
        """rt_merge_async: this context becomes the sample-weighted average of itself and `sources` (contexts of the same size)."""
        srcs = (C.c_void_p * max(len(sources), 1))(*[s._h.value if s is not None else None for s in sources])
        self._check(self._lib.rt_merge_async(self._h, srcs, len(sources), C.c_void_p(stream or 0)))

    # --- frame error on the device (rt_compare.hip) --------------------------------------
    def compare_tiles(self):
        """rt_compare_tiles: (tiles_y, tiles_x) of the tile map of this context's local rows."""
        tx, ty = C.c_int(), C.c_int()
        n = self._lib.rt_compare_tiles(self._h, C.byref(tx), C.byref(ty))
        if n < 0:
            self._check(n)
        return ty.value, tx.value

    def compare(self, other, tiles=False):
        """rt_compare: the error between this context's packed frame and `other`'s as a dict (FrameError.as_dict); with tiles=True
        also the squared error per 8x8 tile, uint32 [tiles_y, tiles_x]."""
        err = FrameError()
        h_other = other._h if other is not None else None
        if not tiles:
            self._check(self._lib.rt_compare(self._h, h_other, C.byref(err), None))
            return err.as_dict()
        tmap = np.zeros(self.compare_tiles(), np.uint32)
        self._check(self._lib.rt_compare(self._h, h_other, C.byref(err), _ptr(tmap)))
        return err.as_dict(), tmap

    def compare_async(self, other, result_ptr, tiles_ptr=None, stream=None):
        """rt_compare_async: queue the comparison on `stream`; `result_ptr` is the device address of 48 bytes (an rt_frame_error),
        `tiles_ptr` the device address of the tile map's words, or None."""
        self._check(self._lib.rt_compare_async(self._h, other._h if other is not None else None, C.c_void_p(result_ptr or 0),
                                               C.c_void_p(tiles_ptr or 0), C.c_void_p(stream or 0)))

    def render_converged(self, other, target_db, passes_per_check, max_passes):
        """rt_render_converged: both contexts rendered in step until the PSNR BETWEEN them reaches `target_db` or they hold
        `max_passes` passes.  Returns (reached, error dict of the last check, number of checks)."""
        err, checks = FrameError(), C.c_int()
        rc = self._lib.rt_render_converged(self._h, other._h if other is not None else None, target_db, passes_per_check, max_passes,
                                           C.byref(err), C.byref(checks))
        if rc < 0:
            self._check(rc)
        return rc == 1, err.as_dict(), checks.value

    # --- adaptive sampling (rt_tiles.hip) --------------------------------------------------
    def tile_passes(self):
        """rt_tile_passes: the pass count of every 8x8 tile, uint32 [tiles_y, tiles_x]."""
        out = np.zeros(self.compare_tiles(), np.uint32)
        self._check(self._lib.rt_tile_passes(self._h, _ptr(out)))
        return out

    def select_tiles(self, err_ptr, above, stream=None):
        """rt_select_tiles: select the groups (32x8 pixels) at the front whose error in the DEVICE map at `err_ptr` lies above `above`
        (None: every group at the front).  Returns (selected groups, the 8x8 tiles they cover)."""
        counts = (C.c_uint32 * 2)()
        self._check(self._lib.rt_select_tiles(self._h, C.c_void_p(err_ptr or 0), above, C.c_void_p(stream or 0), counts))
        return int(counts[0]), int(counts[1])

    def render_tiles_async(self, n_samples, stream=None):
        """rt_render_tiles_async: `n_samples` passes on the selected groups and nothing else."""
        self._check(self._lib.rt_render_tiles_async(self._h, n_samples, C.c_void_p(stream or 0)))

    def render_adaptive(self, other, tile_db, min_passes, passes_per_check, max_passes):
        """rt_render_adaptive: both contexts rendered in step, each group of tiles until the PSNR between its two halves reaches `tile_db`
        or the contexts hold `max_passes` passes.  Returns (every group retired, error dict of the last whole-frame check, number of checks)."""
        err, checks = FrameError(), C.c_int()
        rc = self._lib.rt_render_adaptive(self._h, other._h if other is not None else None, tile_db, min_passes, passes_per_check, max_passes,
                                          C.byref(err), C.byref(checks))
        if rc < 0:
            self._check(rc)
        return rc == 1, err.as_dict(), checks.value

    # --- denoising (rt_denoise.hip) ----------------------------------------------------------
    def denoise(self, a, b, params=None, stream=None):
        """rt_denoise_async: this context's colour plane (the merge of `a` and `b`) filtered by non-local means, steered by the difference of
        the two halves.  `params`: a DenoiseParams, a dict of its fields over the defaults, or None for the defaults."""
        self._check(self._lib.rt_denoise_async(self._h, a._h if a is not None else None, b._h if b is not None else None,
                                               _denoise_params(params), C.c_void_p(stream or 0)))

    # --- the error of the filtered frame (rt_denoise.hip, rt_compare.hip) ------------------------
    def denoise_pair(self, other, params=None, stream=None):
        """rt_denoise_pair_async: this context's colour plane filtered with weights from `other`'s and the reverse, each into a plane its
        context owns beside the colour plane (read_filtered, compare_filtered).  `params` as for denoise()."""
        self._check(self._lib.rt_denoise_pair_async(self._h, other._h if other is not None else None, _denoise_params(params), C.c_void_p(stream or 0)))

    def denoise_pair_tiles(self, other, params=None, stream=None):
        """rt_denoise_pair_tiles_async: denoise_pair() for the groups of the current selection alone -- the planes of the groups that
        render_tiles_async has just rendered made current again, every other pixel kept."""
        self._check(self._lib.rt_denoise_pair_tiles_async(self._h, other._h if other is not None else None, _denoise_params(params), C.c_void_p(stream or 0)))

    # --- feature planes and the guide (rt_features.hip) --------------------------------------------
    def features_async(self, stream=None):
        """rt_features_async: the feature plane of this context's scene and camera, formed on the device (read_features)."""
        self._check(self._lib.rt_features_async(self._h, C.c_void_p(stream or 0)))

    def last_features_kernel(self):
        """Symbol of the kernel the last features_async launched (rt_last_features_kernel): the sweep's, or the hierarchy's by table placement."""
        return self._lib.rt_last_features_kernel(self._h).decode()

    def read_features(self):
        """rt_read_features: the feature plane, float32 [h][w][8] in the colour plane's row order: albedo, normal, distance and -- word 7, view it as
        uint32 -- the scene index (0xFFFFFFFF: the sky)."""
        out = np.zeros((self.h, self.w, 8), np.float32)
        self._check(self._lib.rt_read_features(self._h, _ptr(out)))
        return out

    def set_denoise_guide(self, guide=None):
        """rt_set_denoise_guide: None switches the guide off; a GuideParams or a dict of fields laid over guide_defaults() switches it on."""
        self._check(self._lib.rt_set_denoise_guide(self._h, _guide_params(guide)))

    # --- temporal reprojection (rt_reproject.hip) ---------------------------------------------------
    def reproject_async(self, src, params=None, stream=None):
        """rt_reproject_async: `src`'s history (its temporal plane while current, else its colour plane) carried into this context's view and
        blended with this context's colour plane, into the temporal plane this context owns (read_temporal).  `params`: a ReprojectParams, a
        dict of its fields over the defaults, or None for the defaults."""
        self._check(self._lib.rt_reproject_async(self._h, src._h if src is not None else None, _reproject_params(params), C.c_void_p(stream or 0)))

    def read_temporal(self, packed=True):
        """rt_read_temporal: the temporal plane, float32 [h][w][4] (rgb, n) in the colour plane's row order, and -- packed=True -- its packed
        plane, uint32 [h * w] as read_pixels() lays it out (row 0 = bottom)."""
        rgbn = np.zeros((self.h, self.w, 4), np.float32)
        px = np.zeros(self.h * self.w, np.uint32) if packed else None
        self._check(self._lib.rt_read_temporal(self._h, _ptr(rgbn), _ptr(px) if packed else None))
        return (rgbn, px) if packed else rgbn

    @staticmethod
    def reproject_defaults():
        """rt_reproject_defaults (the module-level reproject_defaults)."""
        return reproject_defaults()

    # --- edge-avoiding wavelet filter (rt_atrous.hip) ----------------------------------------------
    def atrous_async(self, params=None, stream=None):
        """rt_atrous_async: this context's temporal plane while current, else its colour plane, through the a-trous levels into the filtered
        plane this context owns (read_atrous).  `params`: an AtrousParams, a dict of its fields over the defaults, or None for the defaults."""
        self._check(self._lib.rt_atrous_async(self._h, _atrous_params(params), C.c_void_p(stream or 0)))

    def read_atrous(self, packed=True):
        """rt_read_atrous: the filtered plane, float32 [h][w][4] (rgb, variance) in the colour plane's row order, and -- packed=True -- its packed
        plane, uint32 [h * w] as read_pixels() lays it out (row 0 = bottom)."""
        rgbv = np.zeros((self.h, self.w, 4), np.float32)
        px = np.zeros(self.h * self.w, np.uint32) if packed else None
        self._check(self._lib.rt_read_atrous(self._h, _ptr(rgbv), _ptr(px) if packed else None))
        return (rgbv, px) if packed else rgbv

    @staticmethod
    def atrous_defaults():
        """rt_atrous_defaults (the module-level atrous_defaults)."""
        return atrous_defaults()

    # --- temporal luminance moments (rt_reproject.hip, rt_atrous.hip) ------------------------------
    def set_temporal_moments(self, moments=None):
        """rt_set_temporal_moments: None switches the setting off; a MomentsParams or a dict of fields laid over moments_defaults() switches it
        on: reproject_async INTO this context then forms its moments plane too, and atrous_async takes V0 from it (rule 28) while it is current."""
        self._check(self._lib.rt_set_temporal_moments(self._h, _moments_params(moments)))

    def read_moments(self):
        """rt_read_moments: the moments plane, float32 [h][w][4] (m1, m2, k, v) in the colour plane's row order."""
        m = np.zeros((self.h, self.w, 4), np.float32)
        self._check(self._lib.rt_read_moments(self._h, _ptr(m)))
        return m

    @staticmethod
    def moments_defaults():
        """rt_moments_defaults (the module-level moments_defaults)."""
        return moments_defaults()

    # --- shadow-aware history (rt_reproject.hip) -----------------------------------------------
    def set_shadow_history(self, shadow=None):
        """rt_set_shadow_history: None switches the setting off; a ShadowHistoryParams or a dict of fields laid over shadow_history_defaults()
        switches it on: reproject_async INTO this context then caps the history of pixels where a changed record's shadow came or went (rules 29-32)
        and forms the flag plane (read_history_flags)."""
        self._check(self._lib.rt_set_shadow_history(self._h, _shadow_history_params(shadow)))

    def read_history_flags(self):
        """rt_read_history_flags: the flag plane, uint8 [h][w] (0 or 1) in the colour plane's row order."""
        k = np.zeros((self.h, self.w), np.uint8)
        self._check(self._lib.rt_read_history_flags(self._h, _ptr(k)))
        return k

    @staticmethod
    def shadow_history_defaults():
        """rt_shadow_history_defaults (the module-level shadow_history_defaults)."""
        return shadow_history_defaults()

    def read_filtered(self):
        """rt_read_filtered: the cross-filtered plane, float32 [3 * w * h] as read_colors() lays it out."""
        out = np.zeros(3 * self.w * self.h, np.float32)
        self._check(self._lib.rt_read_filtered(self._h, _ptr(out)))
        return out

    def compare_filtered(self, other, tiles=False):
        """rt_compare_filtered: compare() over the packed cross-filtered planes of one denoise_pair call."""
        err = FrameError()
        h_other = other._h if other is not None else None
        if not tiles:
            self._check(self._lib.rt_compare_filtered(self._h, h_other, C.byref(err), None))
            return err.as_dict()
        tmap = np.zeros(self.compare_tiles(), np.uint32)
        self._check(self._lib.rt_compare_filtered(self._h, h_other, C.byref(err), _ptr(tmap)))
        return err.as_dict(), tmap

    def compare_filtered_async(self, other, result_ptr, tiles_ptr=None, stream=None):
        """rt_compare_filtered_async: compare_async() over the packed cross-filtered planes."""
        self._check(self._lib.rt_compare_filtered_async(self._h, other._h if other is not None else None, C.c_void_p(result_ptr or 0),
                                                        C.c_void_p(tiles_ptr or 0), C.c_void_p(stream or 0)))

    def render_converged_filtered(self, other, target_db, passes_per_check, max_passes, params=None):
        """rt_render_converged_filtered: render_converged() with the cross-filtered pair's PSNR -- the estimate for the FILTERED merge -- as
        the check.  Returns (reached, error dict of the last check, number of checks)."""
        err, checks = FrameError(), C.c_int()
        rc = self._lib.rt_render_converged_filtered(self._h, other._h if other is not None else None, target_db, passes_per_check, max_passes,
                                                    _denoise_params(params), C.byref(err), C.byref(checks))
        if rc < 0:
            self._check(rc)
        return rc == 1, err.as_dict(), checks.value

    def render_adaptive_filtered(self, other, tile_db, min_passes, passes_per_check, max_passes, params=None):
        """rt_render_adaptive_filtered: render_adaptive() with the tile map taken from the cross-filtered pair."""
        err, checks = FrameError(), C.c_int()
        rc = self._lib.rt_render_adaptive_filtered(self._h, other._h if other is not None else None, tile_db, min_passes, passes_per_check,
                                                   max_passes, _denoise_params(params), C.byref(err), C.byref(checks))
        if rc < 0:
            self._check(rc)
        return rc == 1, err.as_dict(), checks.value

    def render_adaptive_filtered_tiles(self, other, tile_db, min_passes, passes_per_check, max_passes, params=None):
        """rt_render_adaptive_filtered_tiles: render_adaptive_filtered() whose checks after the first filter only the groups that were just
        rendered.  The same render bit for bit; the error dict sums every group's figure of its own last check."""
        err, checks = FrameError(), C.c_int()
        rc = self._lib.rt_render_adaptive_filtered_tiles(self._h, other._h if other is not None else None, tile_db, min_passes, passes_per_check,
                                                         max_passes, _denoise_params(params), C.byref(err), C.byref(checks))
        if rc < 0:
            self._check(rc)
        return rc == 1, err.as_dict(), checks.value

    def stats(self):
        st = Stats()
        self._check(self._lib.rt_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    # --- sharding helpers ---------------------------------------------------------------
    def local_row_map(self):
        """global row index of every local row, in local order."""
        return local_rows_of(self.h, self.rank, self.nranks, self.tile_rows)


def local_rows_of(h, rank, nranks, tile_rows):
    rows = []
    n_tiles = (h + tile_rows - 1) // tile_rows
    for t in range(rank, n_tiles, nranks):
        rows.extend(range(t * tile_rows, min(h, (t + 1) * tile_rows)))
    return np.asarray(rows, dtype=np.int64)


def deinterleave_rows(full_ptr, gathered_ptr, w, h, nranks, tile_rows, pad_rows, device=0, stream=None):
    """rt_deinterleave_rows on raw device pointers (the gather root's frame assembly)."""
    _check(load_library().rt_deinterleave_rows(C.c_void_p(full_ptr), C.c_void_p(gathered_ptr), w, h, nranks, tile_rows,
                                               pad_rows, device, C.c_void_p(stream or 0)))


class DeviceWords:
    """A uint32 array copied into device memory (tests and tools: a hand-made tile map for select_tiles), through hipMalloc / hipMemcpy of
    the HIP runtime the library itself is linked against -- found among the process's loaded objects, so both share one runtime.
    `ptr` is the device address; the memory is freed by close() or with the object."""

    _hip = None

    @classmethod
    def _runtime(cls):
        if cls._hip is None:
            load_library()
            paths = [line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line]
            if not paths:
                raise RtError(-2, "the HIP runtime is not loaded in this process")
            cls._hip = C.CDLL(paths[0])
        return cls._hip

    def __init__(self, words):
        hip = self._runtime()
        a = np.ascontiguousarray(words, dtype=np.uint32)
        p = C.c_void_p()
        if hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 4))) != 0:
            raise RtError(-3, "hipMalloc of %d bytes failed" % a.nbytes)
        self.ptr, self.size = p.value, a.size
        if a.nbytes and hip.hipMemcpy(C.c_void_p(self.ptr), _ptr(a), C.c_size_t(a.nbytes), 1) != 0:     # hipMemcpyHostToDevice; blocking
            self.close()
            raise RtError(-4, "hipMemcpy to the device failed")

    def close(self):
        if getattr(self, "ptr", None):
            self._hip.hipFree(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_seeds(stream_id, count):
    """rt_stream_seeds: the first `count` words of seed stream `stream_id` (0 = the default stream).  Needs no device."""
    out = np.zeros(count, np.uint32)
    load_library().rt_stream_seeds(stream_id, _ptr(out), count)
    return out


def denoise_defaults():
    """rt_denoise_defaults: DenoiseParams {5, 1, 1.0, 0.45}.  Needs no device."""
    p = DenoiseParams()
    load_library().rt_denoise_defaults(C.byref(p))
    return p


def _denoise_params(params):
    """None (the library's defaults), a DenoiseParams, or a dict of fields laid over the defaults -> what the C call takes."""
    if params is None or isinstance(params, DenoiseParams):
        return C.byref(params) if params is not None else None
    p = denoise_defaults()
    for name, value in dict(params).items():
        if name not in ("search_radius", "patch_radius", "alpha", "k"):
            raise ValueError("rt_denoise_params has no field %r" % name)
        setattr(p, name, value)
    return C.byref(p)


def denoise_planes(merged, a, b, w, h, params=None):
    """rt_denoise_planes: the filter of RtContext.denoise on HOST planes ([h][w][3] float32, as read_colors() returns them); returns the
    filtered plane, float32 [3 * w * h].  Needs no device."""
    planes = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in (merged, a, b)]
    for x in planes:
        if x.size != 3 * w * h:
            raise ValueError("expected %d floats, got %d" % (3 * w * h, x.size))
    out = np.zeros(3 * w * h, np.float32)
    _check(load_library().rt_denoise_planes(_ptr(out), _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]), w, h, _denoise_params(params)))
    return out


def denoise_pair_planes(a, b, w, h, params=None):
    """rt_denoise_pair_planes: the two cross-filtered planes (FA, FB) of HOST planes, float32 [3 * w * h] each.  Needs no device."""
    planes = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in (a, b)]
    for x in planes:
        if x.size != 3 * w * h:
            raise ValueError("expected %d floats, got %d" % (3 * w * h, x.size))
    out_a, out_b = np.zeros(3 * w * h, np.float32), np.zeros(3 * w * h, np.float32)
    _check(load_library().rt_denoise_pair_planes(_ptr(out_a), _ptr(out_b), _ptr(planes[0]), _ptr(planes[1]), w, h, _denoise_params(params)))
    return out_a, out_b


def guide_defaults():
    """rt_guide_defaults: GuideParams {0.15, 0.2, 0.05, 0}.  Needs no device."""
    g = GuideParams()
    load_library().rt_guide_defaults(C.byref(g))
    return g


def _guide_params(guide):
    """None (no guide), a GuideParams, or a dict of fields laid over the defaults -> what the C call takes."""
    if guide is None or isinstance(guide, GuideParams):
        return C.byref(guide) if guide is not None else None
    g = guide_defaults()
    for name, value in dict(guide).items():
        if name not in ("k_albedo", "k_normal", "k_depth", "reserved"):
            raise ValueError("rt_guide_params has no field %r" % name)
        setattr(g, name, value)
    return C.byref(g)


def reproject_defaults():
    """rt_reproject_defaults: ReprojectParams {4.0, 64.0, {0, 0}}.  Needs no device."""
    p = ReprojectParams()
    load_library().rt_reproject_defaults(C.byref(p))
    return p


def _reproject_params(params):
    """None (the library's defaults), a ReprojectParams, or a dict of fields laid over the defaults -> what the C call takes."""
    if params is None or isinstance(params, ReprojectParams):
        return C.byref(params) if params is not None else None
    p = reproject_defaults()
    for name, value in dict(params).items():
        if name not in ("k_pos", "max_history"):
            raise ValueError("rt_reproject_params has no field %r" % name)
        setattr(p, name, value)
    return C.byref(p)


def reproject_planes(dst, src, w, h, params=None):
    """rt_reproject_planes: rules 15-19 on HOST planes; returns the temporal plane, float32 [h][w][4].  `dst` and `src` are dicts, one per side:
    plane ([h][w][3] as read_colors() returns it, or [h][w][4] as read_temporal() does; dst's may be None at passes 0), passes, feat ([h][w][8]),
    cam (15 floats), spheres (records; both sides the same count).  Needs no device."""
    keep, views, count = _reproject_views(dst, src, w, h)
    out = np.zeros((h, w, 4), np.float32)
    _check(load_library().rt_reproject_planes(_ptr(out), C.byref(views[0]), C.byref(views[1]), count, w, h, _reproject_params(params)))
    return out


def _reproject_views(dst, src, w, h):
    """The two rt_reproject_view records of the sides' dicts, the arrays they point into (to be kept alive) and the record count."""
    keep, views = [], []
    count = None
    for side in (dst, src):
        sph = as_spheres(side["spheres"])
        if count is not None and len(sph) != count:
            raise ValueError("the two sides hold %d and %d records" % (count, len(sph)))
        count = len(sph)
        cam = as_camera(side["cam"])
        feat = np.ascontiguousarray(side["feat"], dtype=np.float32).reshape(-1)
        if feat.size != 8 * w * h:
            raise ValueError("a feature plane of %d floats, got %d" % (8 * w * h, feat.size))
        plane, channels = side.get("plane"), 3
        if plane is not None:
            plane = np.ascontiguousarray(plane, dtype=np.float32).reshape(-1)
            if plane.size not in (3 * w * h, 4 * w * h):
                raise ValueError("a plane of %d or %d floats, got %d" % (3 * w * h, 4 * w * h, plane.size))
            channels = plane.size // (w * h)
        keep += [sph, cam, feat, plane]
        views.append(ReprojectView(plane.ctypes.data if plane is not None else None, channels, int(side["passes"]), feat.ctypes.data, cam.ctypes.data,
                                   sph.ctypes.data if count else None))
    return keep, views, count


def moments_defaults():
    """rt_moments_defaults: MomentsParams {4.0, {0, 0, 0}}.  Needs no device."""
    p = MomentsParams()
    load_library().rt_moments_defaults(C.byref(p))
    return p


def _moments_params(params):
    """None, a MomentsParams, or a dict of fields laid over the defaults -> what the C call takes."""
    if params is None or isinstance(params, MomentsParams):
        return C.byref(params) if params is not None else None
    p = moments_defaults()
    for name, value in dict(params).items():
        if name != "k_min":
            raise ValueError("rt_moments_params has no field %r" % name)
        setattr(p, name, value)
    return C.byref(p)


def reproject_moments_planes(dst, src, w, h, src_m=None, params=None):
    """rt_reproject_moments_planes: rules 15-19 and 25-27 on HOST planes; returns (the temporal plane, the moments plane), float32 [h][w][4] each.
    `dst` and `src` as reproject_planes takes them; `src_m` is the source's moments plane [h][w][4], or None for rule 25's luminance of its plane.
    Needs no device."""
    keep, views, count = _reproject_views(dst, src, w, h)
    if src_m is not None:
        src_m = np.ascontiguousarray(src_m, dtype=np.float32).reshape(-1)
        if src_m.size != 4 * w * h:
            raise ValueError("a moments plane of %d floats, got %d" % (4 * w * h, src_m.size))
    out, out_m = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    _check(load_library().rt_reproject_moments_planes(_ptr(out), _ptr(out_m), C.byref(views[0]), C.byref(views[1]), _ptr(src_m) if src_m is not None else None,
                                                      count, w, h, _reproject_params(params)))
    return out, out_m


def shadow_history_defaults():
    """rt_shadow_history_defaults: ShadowHistoryParams {2.0, {0, 0, 0}}.  Needs no device."""
    p = ShadowHistoryParams()
    load_library().rt_shadow_history_defaults(C.byref(p))
    return p


def _shadow_history_params(params):
    """None, a ShadowHistoryParams, or a dict of fields laid over the defaults -> what the C call takes."""
    if params is None or isinstance(params, ShadowHistoryParams):
        return C.byref(params) if params is not None else None
    p = shadow_history_defaults()
    for name, value in dict(params).items():
        if name != "keep":
            raise ValueError("rt_shadow_history_params has no field %r" % name)
        setattr(p, name, value)
    return C.byref(p)


def reproject_shadow_planes(dst, src, w, h, src_m=None, params=None, shadow=None, moments=True):
    """rt_reproject_shadow_planes: rules 15-19, 25-27 and 29-32 on HOST planes; returns (the temporal plane float32 [h][w][4], the moments plane
    float32 [h][w][4] or None with moments=False, the flag plane uint8 [h][w]).  `dst`, `src`, `src_m` and `params` as reproject_moments_planes takes
    them; `shadow`: a ShadowHistoryParams, a dict of its fields over the defaults, or None for no shadow rules (the flags are then all 0).
    Needs no device."""
    keep, views, count = _reproject_views(dst, src, w, h)
    if src_m is not None:
        src_m = np.ascontiguousarray(src_m, dtype=np.float32).reshape(-1)
        if src_m.size != 4 * w * h:
            raise ValueError("a moments plane of %d floats, got %d" % (4 * w * h, src_m.size))
    out, out_m, out_k = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32) if moments else None, np.zeros((h, w), np.uint8)
    _check(load_library().rt_reproject_shadow_planes(_ptr(out), _ptr(out_m) if moments else None, _ptr(out_k), C.byref(views[0]), C.byref(views[1]),
                                                     _ptr(src_m) if src_m is not None else None, count, w, h, _reproject_params(params),
                                                     _shadow_history_params(shadow)))
    return out, out_m, out_k


def shadow_history_pairs(src_spheres, dst_spheres):
    """rt_shadow_history_pairs: rule 29's pair list of the records before (`src_spheres`) and after (`dst_spheres`), int64 [n][2] of (l, j) in rule
    29's order.  Needs no device."""
    s, d = as_spheres(src_spheres), as_spheres(dst_spheres)
    if len(s) != len(d):
        raise ValueError("the two sides hold %d and %d records" % (len(s), len(d)))
    lib = load_library()
    n = lib.rt_shadow_history_pairs(s.ctypes.data if len(s) else None, d.ctypes.data if len(s) else None, len(s), None, 0)
    if n < 0:
        raise RtError(-1, lib.rt_last_error().decode(errors="replace"))
    out = np.zeros((n, 2), np.uint32)
    lib.rt_shadow_history_pairs(s.ctypes.data if len(s) else None, d.ctypes.data if len(s) else None, len(s), _ptr(out) if n else None, n)
    return out.astype(np.int64)


def atrous_defaults():
    """rt_atrous_defaults: AtrousParams {3, 1.5, 0.3, 0}.  Needs no device."""
    p = AtrousParams()
    load_library().rt_atrous_defaults(C.byref(p))
    return p


def _atrous_params(params):
    """None (the library's defaults), an AtrousParams, or a dict of fields laid over the defaults -> what the C call takes."""
    if params is None or isinstance(params, AtrousParams):
        return C.byref(params) if params is not None else None
    p = atrous_defaults()
    for name, value in dict(params).items():
        if name not in ("levels", "k_lum", "k_normal"):
            raise ValueError("rt_atrous_params has no field %r" % name)
        setattr(p, name, value)
    return C.byref(p)


def atrous_planes(plane, feat, w, h, passes=0, params=None):
    """rt_atrous_planes: rules 20-23 on HOST planes; returns the filtered plane, float32 [h][w][4] (rgb, variance).  `plane` is [h][w][3] as
    read_colors() returns it, every pixel at `passes` samples, or [h][w][4] as read_temporal() does; `feat` is [h][w][8].  Needs no device."""
    plane = np.ascontiguousarray(plane, dtype=np.float32).reshape(-1)
    if plane.size not in (3 * w * h, 4 * w * h):
        raise ValueError("a plane of %d or %d floats, got %d" % (3 * w * h, 4 * w * h, plane.size))
    feat = np.ascontiguousarray(feat, dtype=np.float32).reshape(-1)
    if feat.size != 8 * w * h:
        raise ValueError("a feature plane of %d floats, got %d" % (8 * w * h, feat.size))
    out = np.zeros((h, w, 4), np.float32)
    _check(load_library().rt_atrous_planes(_ptr(out), _ptr(plane), plane.size // (w * h), int(passes), _ptr(feat), w, h, _atrous_params(params)))
    return out


def atrous_moments_planes(plane, feat, w, h, passes=0, m=None, params=None, moments=None):
    """rt_atrous_moments_planes: rules 20-23 with rule 28 on HOST planes; returns the filtered plane, float32 [h][w][4] (rgb, variance).  `plane`,
    `feat`, `passes` and `params` as atrous_planes takes them; `m` is the moments plane [h][w][4] (None: rule 21 everywhere); `moments`: a
    MomentsParams, a dict of its fields over the defaults, or None for the defaults.  Needs no device."""
    plane = np.ascontiguousarray(plane, dtype=np.float32).reshape(-1)
    if plane.size not in (3 * w * h, 4 * w * h):
        raise ValueError("a plane of %d or %d floats, got %d" % (3 * w * h, 4 * w * h, plane.size))
    feat = np.ascontiguousarray(feat, dtype=np.float32).reshape(-1)
    if feat.size != 8 * w * h:
        raise ValueError("a feature plane of %d floats, got %d" % (8 * w * h, feat.size))
    if m is not None:
        m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
        if m.size != 4 * w * h:
            raise ValueError("a moments plane of %d floats, got %d" % (4 * w * h, m.size))
    out = np.zeros((h, w, 4), np.float32)
    _check(load_library().rt_atrous_moments_planes(_ptr(out), _ptr(plane), plane.size // (w * h), int(passes), _ptr(m) if m is not None else None, _ptr(feat), w, h,
                                                   _atrous_params(params), _moments_params(moments)))
    return out


def features_planes(spheres, cam, w, h):
    """rt_features_planes: the feature plane of HOST records and a camera, float32 [h][w][8] (RtContext.read_features).  Needs no device."""
    sph = as_spheres(spheres)
    camera = as_camera(cam)
    out = np.zeros((h, w, 8), np.float32)
    _check(load_library().rt_features_planes(_ptr(out), _ptr(sph) if len(sph) else None, len(sph), _ptr(camera), w, h))
    return out


def _feature_plane(feat, w, h, guide):
    if guide is None:
        return None
    f = np.ascontiguousarray(feat, dtype=np.float32).reshape(-1)
    if f.size != 8 * w * h:
        raise ValueError("expected %d floats, got %d" % (8 * w * h, f.size))
    return f


def denoise_guided_planes(merged, a, b, feat, w, h, params=None, guide=None):
    """rt_denoise_guided_planes: denoise_planes under a guide (None: exactly denoise_planes; `feat` is then not read).  Needs no device."""
    planes = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in (merged, a, b)]
    for x in planes:
        if x.size != 3 * w * h:
            raise ValueError("expected %d floats, got %d" % (3 * w * h, x.size))
    f = _feature_plane(feat, w, h, guide)
    out = np.zeros(3 * w * h, np.float32)
    _check(load_library().rt_denoise_guided_planes(_ptr(out), _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2]), _ptr(f) if f is not None else None, w, h,
                                                   _denoise_params(params), _guide_params(guide)))
    return out


def denoise_pair_guided_planes(a, b, feat, w, h, params=None, guide=None):
    """rt_denoise_pair_guided_planes: denoise_pair_planes under a guide (None: exactly denoise_pair_planes).  Needs no device."""
    planes = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in (a, b)]
    for x in planes:
        if x.size != 3 * w * h:
            raise ValueError("expected %d floats, got %d" % (3 * w * h, x.size))
    f = _feature_plane(feat, w, h, guide)
    out_a, out_b = np.zeros(3 * w * h, np.float32), np.zeros(3 * w * h, np.float32)
    _check(load_library().rt_denoise_pair_guided_planes(_ptr(out_a), _ptr(out_b), _ptr(planes[0]), _ptr(planes[1]), _ptr(f) if f is not None else None, w, h,
                                                        _denoise_params(params), _guide_params(guide)))
    return out_a, out_b


def error_psnr(err):
    """rt_error_psnr of a FrameError or of the dict its as_dict() gives: the PSNR over the packed 8-bit channels.  Needs no device."""
    if not isinstance(err, FrameError):
        err = FrameError.from_dict(err)
    return load_library().rt_error_psnr(C.byref(err))


def build_id(diag=False):
    """rt_build_id(): the identity of the sources and flags the loaded library was built from."""
    return load_library(diag).rt_build_id().decode()


def instance_mode(kernel_symbol):
    """The rt_set_mode value of the diagnostics library that selects the instance with this kernel symbol
    (rt_debug_instance: rows of the instance tables are found by name, never by number)."""
    lib = load_library(diag=True)
    mode = lib.rt_debug_instance(kernel_symbol.encode())
    if mode < 0:
        raise RtError(mode, lib.rt_last_error().decode(errors="replace"))
    return mode


def instance_names(fast=False):
    """Kernel symbols of every instance of the diagnostics library's parity (or fast) table, in row order."""
    lib = load_library(diag=True)
    return [lib.rt_debug_instance_name(1 if fast else 0, k).decode() for k in range(lib.rt_debug_variant_count(1 if fast else 0))]


def debug_eval(op, values):
    lib = load_library(diag=True)
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros_like(v)
    _check(lib.rt_debug_eval(op, _ptr(v), _ptr(out), v.size), lib)
    return out
