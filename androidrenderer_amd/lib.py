"""ctypes binding of libsah_hip.so (the C ABI in include/sah_hip.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded this module raises, and every
entry point raises SahError on a non-zero status."""
import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SAH_HIP_LIBRARY") or os.path.join(_HERE, "libsah_hip.so")  # override: A/B builds of the same library


class SahError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"sah status {status}: {message}")
        self.status = status


_lib = None

# every symbol include/sah_hip.h declares
EXPORTS = ["sah_abi_version", "sah_status_string", "sah_last_error", "sah_create", "sah_destroy", "sah_comm_unique_id", "sah_set_stream",
           "sah_sync", "sah_lighting", "sah_copy_scene", "sah_copy_scene_rows", "sah_copy_scene_bloom_mip0_rows", "sah_bloom", "sah_bloom_mip0_rows", "sah_bloom_from_mip0", "sah_bloom_mip_rows", "sah_bloom_from_mip", "sah_bloom_source_rows", "sah_tonemap", "sah_tonemap_ex", "sah_lpv_clear", "sah_lpv_propagate", "sah_probe_notify_updated",
           "sah_sky_update_luts", "sah_ao_clear", "sah_probe_copy", "sah_probe_update", "sah_shadow_render", "sah_gbuffer_render", "sah_rsm_render", "sah_lpv_extract_vpls",
           "sah_lpv_inject_vpls", "sah_rt_build", "sah_rtao", "sah_sun_shadow_mask", "sah_probe_trace", "sah_rtgi_trace", "sah_rt_set_rows", "sah_rt_set_bounces", "sah_debug_rt_structure", "sah_debug_raster_last_pass", "sah_allgather_rows", "sah_allgather_rows_reversed", "sah_allgather_bytes", "sah_comm_set_stream", "sah_comm_wait",
           "sah_ipc_open", "sah_ipc_connect", "sah_ipc_export", "sah_ipc_register", "sah_ipc_unregister", "sah_ipc_reset",
           "sah_chain_create", "sah_chain_submit", "sah_chain_flush", "sah_chain_counts", "sah_chain_destroy"]

# the LPV geometry volume's entries: exported, declared in include/sah_lpv_gv.h (not sah_hip.h)
GV_EXPORTS = ["sah_lpv_inject_rsm_gv", "sah_lpv_inject_scene_gv", "sah_lpv_propagate_gv"]

# the motion-vectors pass: exported, declared in include/sah_motion_vectors.h (not sah_hip.h)
MV_EXPORTS = ["sah_motion_vectors_render"]

# the fused G-buffer + motion-vectors pass: exported, declared in include/sah_gbuffer_motion.h (not sah_hip.h)
GBUFFER_MOTION_EXPORTS = ["sah_gbuffer_motion_render"]

# the VRSAA passes: exported, declared in include/sah_vrsaa.h (not sah_hip.h)
VRSAA_EXPORTS = ["sah_vrsaa_measure_aliasing", "sah_vrsaa_shading_rate_image"]

# temporal anti-aliasing: exported, declared in include/sah_taa.h (not sah_hip.h)
TAA_EXPORTS = ["sah_taa_resolve"]

# temporal upscaling: exported, declared in include/sah_taa_upscale.h (not sah_hip.h)
TAA_UPSCALE_EXPORTS = ["sah_taa_upscale"]

# screen-space ambient occlusion: exported, declared in include/sah_ssao.h (not sah_hip.h)
SSAO_EXPORTS = ["sah_ssao"]

# the filter for the ray-traced masks: exported, declared in include/sah_rt_denoise.h (not sah_hip.h)
RT_DENOISE_EXPORTS = ["sah_rt_denoise"]

# the filter for the RTGI ray planes: exported, declared in include/sah_rtgi_denoise.h (not sah_hip.h)
RTGI_DENOISE_EXPORTS = ["sah_rtgi_denoise"]

# histogram auto-exposure: exported, declared in include/sah_exposure.h (not sah_hip.h)
EXPOSURE_EXPORTS = ["sah_exposure_meter", "sah_exposure_apply"]
EXPOSURE_WORK_BYTES = 1040    # SAH_EXPOSURE_WORK_BYTES
EXPOSURE_BINS = 256           # SAH_EXPOSURE_BINS

# contrast-adaptive sharpening: exported, declared in include/sah_sharpen.h (not sah_hip.h)
SHARPEN_EXPORTS = ["sah_sharpen"]

# screen-space reflections: exported, declared in include/sah_ssr.h (not sah_hip.h)
SSR_EXPORTS = ["sah_ssr"]

# camera motion blur: exported, declared in include/sah_motion_blur.h (not sah_hip.h)
MOTION_BLUR_EXPORTS = ["sah_motion_blur"]
MOTION_BLUR_TILE = 16         # SAH_MOTION_BLUR_TILE

# volumetric sun light: exported, declared in include/sah_sun_shafts.h (not sah_hip.h)
SUN_SHAFTS_EXPORTS = ["sah_sun_shafts"]
SUN_SHAFTS_MAX_STEPS = 64     # SAH_SUN_SHAFTS_MAX_STEPS

# variable-rate lighting and the VRSAA resolve: exported, declared in include/sah_vrs.h (not sah_hip.h)
VRS_EXPORTS = ["sah_lighting_vrs", "sah_vrsaa_resolve"]

# alpha-blended geometry over the lit scene: exported, declared in include/sah_translucent.h (not sah_hip.h)
TRANSLUCENT_EXPORTS = ["sah_translucent_render"]

# the mip-chain generator: exported, declared in include/sah_mip_chain.h (not sah_hip.h)
MIP_CHAIN_EXPORTS = ["sah_mip_chain_generate"]
MIP_CHAIN_MAX_LEVELS = 12     # SAH_MIP_CHAIN_MAX_LEVELS
MIP_CHAIN_MAX_SOURCE = 4096   # SAH_MIP_CHAIN_MAX_SOURCE

# the refit of the acceleration structure: exported, declared in include/sah_rt_refit.h (not sah_hip.h)
RT_REFIT_EXPORTS = ["sah_rt_refit"]

# the LPV mesh lights' entries: exported, declared in include/sah_lpv_mesh_lights.h (not sah_hip.h)
ML_EXPORTS = ["sah_mesh_point_cloud", "sah_lpv_emissive_vpls", "sah_lpv_inject_emissive"]
POINT_CLOUD_ON_SURFACE = 1    # SAH_POINT_CLOUD_ON_SURFACE
EMISSIVE_MATERIAL_ZERO = 1    # SAH_EMISSIVE_MATERIAL_ZERO
LPV_EMISSIVE_MAX_ENTRIES = 1 << 24

# sah_debug_rt_structure: header words, levels in its two tables, the 48-byte triangle record (SAH_RT_STRUCTURE_HEADER_WORDS, ...)
RT_STRUCTURE_HEADER_WORDS = 34
RT_MAX_LEVELS = 15


RT_TRIANGLE = np.dtype([("v0", np.float32, 3), ("primitive", np.uint32), ("v1", np.float32, 3), ("triangle", np.uint32), ("v2", np.float32, 3),
                        ("flags", np.uint32)])
assert RT_TRIANGLE.itemsize == 48


class EmissiveCloud(C.Structure):  # sah_emissive_cloud
    _fields_ = [("vpls", C.c_void_p), ("count", C.c_uint32), ("primitive", C.c_uint32), ("bounds_min", C.c_float * 3), ("bounds_max", C.c_float * 3)]


class LpvCascadeBounds(C.Structure):  # sah_lpv_cascade_bounds
    _fields_ = [("min_bounds", C.c_float * 3), ("max_bounds", C.c_float * 3)]


def mesh_point_cloud(positions, vertex_data, indices, first_index, index_count, vertex_offset, seed, flags=0):
    """sah_mesh_point_cloud on host arrays (positions (N, 3) float32, vertex_data of mesh.VERTEX_DATA, indices uint32): returns
    (positions (n, 3) float32, points of mesh.VERTEX_DATA, bounds_min, bounds_max)."""
    import numpy as np
    from . import mesh
    lib = load()
    pos = np.ascontiguousarray(positions, np.float32)
    vd = np.ascontiguousarray(vertex_data)
    idx = np.ascontiguousarray(indices, np.uint32)
    count, lo, hi = C.c_uint32(0), (C.c_float * 3)(), (C.c_float * 3)()
    args = (pos.ctypes.data if pos.size else None, vd.ctypes.data if vd.size else None, pos.shape[0], idx.ctypes.data if idx.size else None, idx.shape[0],
            first_index, index_count, vertex_offset, seed, flags)
    rc = lib.sah_mesh_point_cloud(*args, None, None, 0, C.byref(count), lo, hi)
    if rc != _abi.SAH_OK:
        raise SahError(rc, f"sah_mesh_point_cloud: {lib.sah_status_string(rc).decode()}")
    out_pos = np.zeros((count.value, 3), np.float32)
    out_vd = np.zeros(count.value, mesh.VERTEX_DATA)
    if count.value:
        rc = lib.sah_mesh_point_cloud(*args, out_pos.ctypes.data, out_vd.ctypes.data, count.value, C.byref(count), lo, hi)
        if rc != _abi.SAH_OK:
            raise SahError(rc, f"sah_mesh_point_cloud: {lib.sah_status_string(rc).decode()}")
    return out_pos, out_vd, np.array(lo[:], np.float32), np.array(hi[:], np.float32)


def load():
    """Loads the library (building is a separate, explicit step: python -m androidrenderer_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found — build it with `python -m androidrenderer_amd.build` (needs hipcc); "
                          "there is no CPU fallback for the product path")
    lib = C.CDLL(LIB_PATH)
    lib.sah_abi_version.restype = C.c_int
    lib.sah_status_string.restype = C.c_char_p
    lib.sah_status_string.argtypes = [C.c_int]
    lib.sah_last_error.restype = C.c_char_p
    lib.sah_last_error.argtypes = [C.c_void_p]
    lib.sah_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.sah_destroy.argtypes = [C.c_void_p]
    lib.sah_destroy.restype = None
    lib.sah_debug_create_detached.argtypes = [C.POINTER(C.c_void_p)]
    lib.sah_comm_unique_id.argtypes = [C.c_void_p]
    lib.sah_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.sah_sync.argtypes = [C.c_void_p]
    lib.sah_debug_deferred_pixels.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.sah_debug_copy_rebuilds.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.sah_debug_cache_epoch.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.sah_debug_lighting_dispatch.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.sah_lighting.argtypes = [C.c_void_p, C.POINTER(_abi.LightingDesc)]
    lib.sah_copy_scene.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.Plane)]
    lib.sah_copy_scene_rows.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.c_uint32, C.c_uint32]
    lib.sah_bloom.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.MipChain)]
    lib.sah_copy_scene_bloom_mip0_rows.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.POINTER(_abi.MipChain)] + [C.c_uint32] * 4
    lib.sah_bloom_mip0_rows.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.MipChain), C.c_uint32, C.c_uint32]
    lib.sah_bloom_from_mip0.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.MipChain)]
    lib.sah_bloom_mip_rows.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.MipChain), C.c_uint32, C.c_uint32, C.c_uint32]
    lib.sah_bloom_from_mip.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.MipChain), C.c_uint32]
    lib.sah_bloom_source_rows.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)]
    lib.sah_tonemap.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.MipChain), C.POINTER(_abi.Plane), C.c_uint32, C.c_uint32]
    lib.sah_tonemap_ex.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.MipChain), C.POINTER(_abi.Plane), C.c_uint32, C.c_uint32, C.c_uint32]
    lib.sah_lpv_clear.argtypes = [C.c_void_p] + [C.POINTER(_abi.Volume)] * 4 + [C.c_uint32]
    lib.sah_lpv_propagate.argtypes = [C.c_void_p, C.POINTER(_abi.Volume), C.POINTER(_abi.Volume), C.c_uint32, C.c_uint32]
    lib.sah_allgather_rows.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.c_uint32, C.c_uint32]
    lib.sah_allgather_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.sah_allgather_rows_reversed.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.c_uint32, C.c_uint32]
    lib.sah_comm_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.sah_comm_wait.argtypes = [C.c_void_p]
    lib.sah_ao_clear.argtypes = [C.c_void_p, C.POINTER(_abi.Plane)]
    lib.sah_sky_update_luts.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.POINTER(C.c_float)]
    lib.sah_probe_copy.argtypes =[C.c_void_p, C.POINTER(_abi.ProbeAtlases), C.POINTER(_abi.ProbeAtlases), C.POINTER(C.c_float * 3)]
    lib.sah_probe_update.argtypes = [C.c_void_p, C.POINTER(_abi.ProbeAtlases), C.POINTER(_abi.Volume), C.c_void_p, C.c_uint32]
    lib.sah_probe_notify_updated.argtypes = [C.c_void_p, C.POINTER(_abi.Volume), C.c_void_p, C.c_uint32]
    lib.sah_shadow_render.argtypes = [C.c_void_p, C.POINTER(_abi.SceneGeometry), C.POINTER(_abi.SunLightConstants), C.c_uint32,
                                      C.POINTER(_abi.Volume), C.c_void_p]
    lib.sah_gbuffer_render.argtypes = [C.c_void_p, C.POINTER(_abi.SceneGeometry), C.POINTER(_abi.ViewData), C.POINTER(_abi.GBuffer), C.c_void_p]
    lib.sah_motion_vectors_render.argtypes = [C.c_void_p, C.POINTER(_abi.SceneGeometry), C.POINTER(_abi.ViewData), C.POINTER(_abi.Plane), C.POINTER(_abi.Plane),
                                              C.c_void_p]
    lib.sah_gbuffer_motion_render.argtypes = [C.c_void_p, C.POINTER(_abi.SceneGeometry), C.POINTER(_abi.ViewData), C.POINTER(_abi.GBuffer), C.POINTER(_abi.Plane),
                                              C.c_void_p]
    lib.sah_rsm_render.argtypes = [C.c_void_p, C.POINTER(_abi.SceneGeometry), C.POINTER(_abi.SunLightConstants), C.POINTER(_abi.LpvCascadeMatrices),
                                   C.c_uint32, C.POINTER(_abi.RsmTargets), C.c_void_p]
    lib.sah_lpv_extract_vpls.argtypes = [C.c_void_p, C.POINTER(_abi.RsmTargets), C.POINTER(_abi.LpvCascadeMatrices), C.c_uint32, C.c_float, C.c_void_p,
                                         C.c_void_p]
    lib.sah_lpv_inject_vpls.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(_abi.LpvCascadeMatrices), C.c_uint32, C.c_uint32,
                                        C.POINTER(_abi.Volume)]
    lib.sah_rt_build.argtypes = [C.c_void_p, C.POINTER(_abi.SceneGeometry), C.POINTER(C.c_uint32)]
    lib.sah_rtao.argtypes = [C.c_void_p, C.POINTER(_abi.ViewData), C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.c_uint32, C.c_float,
                             C.POINTER(_abi.Plane)]
    lib.sah_sun_shadow_mask.argtypes = [C.c_void_p, C.POINTER(_abi.ViewData), C.POINTER(_abi.SunLightConstants), C.POINTER(_abi.Plane), C.POINTER(_abi.Plane),
                                        C.POINTER(_abi.Plane), C.POINTER(_abi.Plane)]
    lib.sah_rt_set_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.sah_rt_set_bounces.argtypes = [C.c_void_p, C.c_uint32]
    lib.sah_debug_rt_structure.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    lib.sah_debug_raster_last_pass.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.sah_probe_trace.argtypes = [C.c_void_p, C.POINTER(_abi.ProbeTraceDesc)]
    lib.sah_rtgi_trace.argtypes = [C.c_void_p, C.POINTER(_abi.ViewData), C.POINTER(_abi.SunLightConstants), C.POINTER(_abi.SkyLuts)] + [C.POINTER(_abi.Plane)] * 5
    lib.sah_ipc_open.argtypes = [C.c_void_p, C.c_void_p]
    lib.sah_ipc_connect.argtypes = [C.c_void_p, C.c_void_p]
    lib.sah_ipc_export.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.sah_ipc_register.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.sah_ipc_unregister.argtypes = [C.c_void_p, C.c_void_p]
    lib.sah_ipc_reset.argtypes = [C.c_void_p]
    lib.sah_chain_create.argtypes = [C.c_void_p, C.POINTER(_abi.ChainPlan), C.POINTER(_abi.ChainFrame), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_void_p)]
    lib.sah_chain_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sah_chain_flush.argtypes = [C.c_void_p]
    lib.sah_chain_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sah_chain_destroy.argtypes = [C.c_void_p]
    lib.sah_debug_chain_graphs.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.sah_chain_destroy.restype = None
    lib.sah_debug_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.sah_lpv_inject_rsm_gv.argtypes = [C.c_void_p, C.POINTER(_abi.RsmTargets), C.POINTER(_abi.LpvCascadeMatrices), C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(_abi.Volume)]
    lib.sah_lpv_inject_scene_gv.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.POINTER(_abi.ViewData),
                                            C.POINTER(_abi.LpvCascadeMatrices), C.c_uint32, C.POINTER(_abi.Volume)]
    lib.sah_mesh_point_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint64,
                                         C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                         C.POINTER(C.c_float)]
    lib.sah_lpv_emissive_vpls.argtypes = [C.c_void_p, C.POINTER(_abi.SceneGeometry), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                          C.c_void_p]
    lib.sah_lpv_inject_emissive.argtypes = [C.c_void_p, C.POINTER(_abi.SceneGeometry), C.POINTER(EmissiveCloud), C.c_uint32,
                                            C.POINTER(_abi.LpvCascadeMatrices), C.POINTER(LpvCascadeBounds), C.c_uint32, C.POINTER(_abi.Volume)]
    lib.sah_lpv_propagate_gv.argtypes = [C.c_void_p, C.POINTER(_abi.Volume), C.POINTER(_abi.Volume), C.POINTER(_abi.Volume), C.c_uint32, C.c_uint32]
    lib.sah_vrsaa_measure_aliasing.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.c_uint32, C.c_uint32]
    lib.sah_vrsaa_shading_rate_image.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.POINTER(_abi.ShadingRateParams)]
    lib.sah_taa_resolve.argtypes = [C.c_void_p] + [C.POINTER(_abi.Plane)] * 5 + [C.POINTER(_abi.TaaParams), C.c_uint32, C.c_uint32]
    lib.sah_taa_upscale.argtypes = [C.c_void_p] + [C.POINTER(_abi.Plane)] * 5 + [C.POINTER(_abi.TaaUpscaleParams), C.c_uint32, C.c_uint32]
    lib.sah_ssao.argtypes = [C.c_void_p, C.POINTER(_abi.ViewData)] + [C.POINTER(_abi.Plane)] * 4 + [C.POINTER(_abi.SsaoParams), C.c_uint32, C.c_uint32]
    lib.sah_rt_denoise.argtypes = [C.c_void_p, C.POINTER(_abi.ViewData), C.POINTER(_abi.RtDenoiseDesc), C.POINTER(_abi.RtDenoiseParams), C.c_uint32, C.c_uint32]
    lib.sah_rtgi_denoise.argtypes = [C.c_void_p, C.POINTER(_abi.ViewData), C.POINTER(_abi.RtgiDenoiseDesc), C.POINTER(_abi.RtgiDenoiseParams), C.c_uint32, C.c_uint32]
    lib.sah_exposure_meter.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.ExposureParams)]
    lib.sah_exposure_apply.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.c_void_p, C.POINTER(_abi.Plane), C.c_uint32, C.c_uint32]
    lib.sah_sharpen.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.SharpenParams), C.c_uint32, C.c_uint32]
    lib.sah_ssr.argtypes = [C.c_void_p, C.POINTER(_abi.ViewData)] + [C.POINTER(_abi.Plane)] * 8 + [C.POINTER(_abi.SsrParams), C.c_uint32, C.c_uint32]
    lib.sah_motion_blur.argtypes = [C.c_void_p] + [C.POINTER(_abi.Plane)] * 5 + [C.POINTER(_abi.MotionBlurParams), C.c_uint32, C.c_uint32]
    lib.sah_sun_shafts.argtypes = [C.c_void_p, C.POINTER(_abi.ViewData), C.POINTER(_abi.SunLightConstants), C.POINTER(_abi.Volume)] + [C.POINTER(_abi.Plane)] * 4 + \
                                  [C.POINTER(_abi.SunShaftsParams), C.c_uint32, C.c_uint32]
    lib.sah_lighting_vrs.argtypes = [C.c_void_p, C.POINTER(_abi.LightingVrsDesc)]
    lib.sah_translucent_render.argtypes = [C.c_void_p, C.POINTER(_abi.TranslucentDesc)]
    lib.sah_vrsaa_resolve.argtypes = [C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.c_uint32, C.c_uint32]
    lib.sah_mip_chain_generate.argtypes =[C.c_void_p, C.POINTER(_abi.Plane), C.POINTER(_abi.Plane), C.c_uint32]
    lib.sah_rt_refit.argtypes = [C.c_void_p, C.POINTER(_abi.SceneGeometry), C.c_void_p]
    _lib = lib
    return lib


def create_detached():
    """Test hook (sah_debug_create_detached): the handle (c_void_p) of a context with no device behind it, for the caller to sah_destroy — or
    None where a HIP device is present: there the library refuses, because what is thrown at such a context must never reach a GPU."""
    lib = load()
    h = C.c_void_p()
    rc = lib.sah_debug_create_detached(C.byref(h))
    if rc == _abi.SAH_ERR_UNSUPPORTED:
        return None
    if rc != _abi.SAH_OK or not h.value:
        raise SahError(rc, f"sah_debug_create_detached: {lib.sah_status_string(rc).decode()}")
    return h


class Context:
    """One sah_ctx: a device, a stream, optionally an RCCL communicator."""

    def __init__(self, device=0, rank=0, world=1, comm_id=None, stream=None):
        self.lib = load()
        h = C.c_void_p()
        idbuf = None
        if comm_id is not None:
            idbuf = C.create_string_buffer(bytes(comm_id), 128)
        rc = self.lib.sah_create(C.byref(h), device, rank, world, idbuf)
        if rc != _abi.SAH_OK:
            raise SahError(rc, self.lib.sah_status_string(rc).decode())
        self.handle = h
        if stream is not None:
            self.set_stream(stream)

    def _check(self, rc):
        if rc != _abi.SAH_OK:
            msg = self.lib.sah_last_error(self.handle).decode() or self.lib.sah_status_string(rc).decode()
            raise SahError(rc, msg)

    def set_stream(self, hip_stream_handle):
        self._check(self.lib.sah_set_stream(self.handle, C.c_void_p(hip_stream_handle)))

    STRAYS_MODES = {"auto": _abi.DEBUG_STRAYS_AUTO, "launch": _abi.DEBUG_STRAYS_LAUNCH, "inline": _abi.DEBUG_STRAYS_INLINE}

    def debug_set(self, force_general=False, force_ppt=0, strays="auto"):
        """Testing hook: run the general kernel instead of the fast one / force pixels-per-thread / say how the fast kernel's strays (the
        pixels it lists for the general restatement) are finished: "auto" by the context's record of recent calls, "launch" always by the
        fix-up launch, "inline" always by the fast kernel itself where its body can (one with a sky bound)."""
        if strays not in self.STRAYS_MODES:
            raise ValueError(f"strays must be one of {tuple(self.STRAYS_MODES)}, not {strays!r}")
        self._check(self.lib.sah_debug_set(self.handle, int(force_general), int(force_ppt), self.STRAYS_MODES[strays]))

    def deferred_pixels(self):
        """Analysis hook: pixels the last fast-path lighting call handed to the fix-up kernel (synchronises)."""
        n = C.c_uint64()
        self._check(self.lib.sah_debug_deferred_pixels(self.handle, C.byref(n)))
        return int(n.value)

    def copy_rebuilds(self):
        """Test hook: (full rebuilds of the LPV gather copy, of the fp32 irradiance copy) by lighting() since the context was made."""
        out = (C.c_uint32 * 2)()
        self._check(self.lib.sah_debug_copy_rebuilds(self.handle, out))
        return int(out[0]), int(out[1])

    def cache_epoch(self):
        """Test hook: the context's cache epoch — it moves when something changes that a launch depends on beyond its arguments (a context
        buffer reallocated, a table rebuilt, a gather copy dropped or rebuilt); captured graphs are replayed only while it stands."""
        e = C.c_uint64()
        self._check(self.lib.sah_debug_cache_epoch(self.handle, C.byref(e)))
        return int(e.value)

    DISPATCH_FIELDS = ("family", "ppt", "pos_div_nr", "ncasc_pow2", "row_magic", "sky_ratio", "sky_workgroups", "tiled_fast_geom", "tiled_fast_lpv",
                       "repack", "table_rebuilt", "pos_div_shared", "strays")

    def lighting_dispatch(self):
        """Test hook: what the last lighting() call of this context decided, as a dict — family ('general' / 'fast' / 'tiled'), ppt, pos_div_nr,
        ncasc_pow2, row_magic (1: the multiply-high row split), sky_ratio, sky_workgroups (leading the grid), tiled_fast_geom, tiled_fast_lpv,
        repack, table_rebuilt, pos_div_shared (1: the position divides shared one reciprocal through the condition for zeros of either sign in the
        inverse projection; 0 where pos_div_nr is 1).  Recorded on the host: no device work, no synchronisation — except for pos_div_shared where
        the host's half of its condition held: the kernel decides from a word the table's build leaves on the device, which is then fetched.
        strays: how the fast kernel's listed pixels were finished — 'launch' (the fix-up launch followed), 'inline' (the fast kernel shaded them
        itself: one launch), None where the fast kernel did not run."""
        out = (C.c_uint32 * len(self.DISPATCH_FIELDS))()
        self._check(self.lib.sah_debug_lighting_dispatch(self.handle, out))
        rep = {k: int(v) for k, v in zip(self.DISPATCH_FIELDS, out)}
        rep["family"] = ("general", "fast", "tiled")[rep["family"]]
        rep["strays"] = (None, "launch", "inline")[rep["strays"]]
        return rep

    def sync(self):
        self._check(self.lib.sah_sync(self.handle))

    def lighting(self, desc):
        self._check(self.lib.sah_lighting(self.handle, C.byref(desc)))

    def copy_scene(self, lit, out, row_begin=0, row_end=0):
        self._check(self.lib.sah_copy_scene_rows(self.handle, C.byref(lit), C.byref(out), row_begin, row_end))

    def copy_scene_bloom_mip0(self, lit, out, chain, aa_rows=(0, 0), mip_rows=(0, 0)):
        """Copy scene + bloom mip 0 in one pass over lit (rows of `antialiased`, rows of mip 0; (0, 0) = all)."""
        self._check(self.lib.sah_copy_scene_bloom_mip0_rows(self.handle, C.byref(lit), C.byref(out), C.byref(chain), aa_rows[0], aa_rows[1], mip_rows[0], mip_rows[1]))

    def bloom(self, scene, chain):
        self._check(self.lib.sah_bloom(self.handle, C.byref(scene), C.byref(chain)))

    def bloom_mip0_rows(self, scene, chain, row_begin, row_end):
        self._check(self.lib.sah_bloom_mip0_rows(self.handle, C.byref(scene), C.byref(chain), row_begin, row_end))

    def bloom_mip_rows(self, scene, chain, mip, row_begin, row_end):
        """rows of mip `mip` from its source (the scene for mip 0, mip - 1 otherwise)"""
        self._check(self.lib.sah_bloom_mip_rows(self.handle, C.byref(scene), C.byref(chain), mip, row_begin, row_end))

    def bloom_from_mip(self, scene, chain, mip):
        """mips mip + 1 .. from mip `mip`"""
        self._check(self.lib.sah_bloom_from_mip(self.handle, C.byref(scene), C.byref(chain), mip))

    def bloom_from_mip0(self, scene, chain):
        self._check(self.lib.sah_bloom_from_mip0(self.handle, C.byref(scene), C.byref(chain)))

    def tonemap(self, scene, chain, out, row_begin=0, row_end=0, flags=0):
        """flags: 0 = strict (bit-identical to the oracle), _abi.TONEMAP_TOLERANCE_1CODE = within one code of it, about twice as fast"""
        self._check(self.lib.sah_tonemap_ex(self.handle, C.byref(scene), C.byref(chain), C.byref(out), row_begin, row_end, flags))

    def lpv_clear(self, red, green, blue, geometry, num_cascades):
        null = C.POINTER(_abi.Volume)()
        args = [C.byref(v) if v is not None else null for v in (red, green, blue, geometry)]
        self._check(self.lib.sah_lpv_clear(self.handle, *args, num_cascades))

    def lpv_propagate(self, a_rgb, b_rgb, num_cascades, steps):
        a = (_abi.Volume * 3)(*a_rgb)
        b = (_abi.Volume * 3)(*b_rgb)
        self._check(self.lib.sah_lpv_propagate(self.handle, a, b, num_cascades, steps))

    def lpv_inject_rsm_gv(self, rsm, cascades, first_cascade, cascade_count, num_cascades, geometry):
        """sah_lpv_inject_rsm_gv: rsm an _abi.RsmTargets, cascades an (_abi.LpvCascadeMatrices * n) array"""
        self._check(self.lib.sah_lpv_inject_rsm_gv(self.handle, C.byref(rsm), cascades, first_cascade, cascade_count, num_cascades, C.byref(geometry)))

    def lpv_inject_scene_gv(self, depth, normals, view, cascades, num_cascades, geometry):
        self._check(self.lib.sah_lpv_inject_scene_gv(self.handle, C.byref(depth), C.byref(normals), C.byref(view), cascades, num_cascades, C.byref(geometry)))

    def lpv_propagate_gv(self, a_rgb, b_rgb, geometry, num_cascades, steps):
        """sah_lpv_propagate_gv; geometry None = sah_lpv_propagate"""
        a = (_abi.Volume * 3)(*a_rgb)
        b = (_abi.Volume * 3)(*b_rgb)
        g = C.byref(geometry) if geometry is not None else C.POINTER(_abi.Volume)()
        self._check(self.lib.sah_lpv_propagate_gv(self.handle, a, b, g, num_cascades, steps))

    def lpv_emissive_vpls(self, geometry, primitive_index, positions_ptr, points_ptr, num_points, flags, out_ptr):
        """sah_lpv_emissive_vpls: geometry an _abi.SceneGeometry over device arrays; the three pointers are device addresses"""
        self._check(self.lib.sah_lpv_emissive_vpls(self.handle, C.byref(geometry), primitive_index, C.c_void_p(positions_ptr), C.c_void_p(points_ptr),
                                                   num_points, flags, C.c_void_p(out_ptr)))

    def lpv_inject_emissive(self, geometry, clouds, cascades, bounds, num_cascades, a_rgb):
        """sah_lpv_inject_emissive: clouds a sequence of EmissiveCloud, bounds an (LpvCascadeBounds * n) array"""
        table = (EmissiveCloud * max(len(clouds), 1))(*clouds)
        a = (_abi.Volume * 3)(*a_rgb)
        self._check(self.lib.sah_lpv_inject_emissive(self.handle, C.byref(geometry), table, len(clouds), cascades, bounds, num_cascades, a))

    def sky_update_luts(self, transmittance, multiscattering, sky_view, light_vector):
        lv = (C.c_float * 3)(*[float(v) for v in light_vector])
        self._check(self.lib.sah_sky_update_luts(self.handle, C.byref(transmittance), C.byref(multiscattering), C.byref(sky_view), lv))

    def ao_clear(self, ao):
        self._check(self.lib.sah_ao_clear(self.handle, C.byref(ao)))

    def probe_copy(self, src, dst, cascade_movement):
        """src, dst: _abi.ProbeAtlases; cascade_movement: 4 x 3 floats (probe cells per cascade)."""
        mv = ((C.c_float * 3) * 4)(*[(C.c_float * 3)(*[float(v) for v in row]) for row in cascade_movement])
        self._check(self.lib.sah_probe_copy(self.handle, C.byref(src), C.byref(dst), mv))

    def probe_update(self, atlases, trace_results, probes_to_update_ptr, num_probes):
        """probes_to_update_ptr: device address of num_probes packed uint32 triples."""
        self._check(self.lib.sah_probe_update(self.handle, C.byref(atlases), C.byref(trace_results), C.c_void_p(probes_to_update_ptr), num_probes))

    def probe_notify_updated(self, probe_irradiance, probes_ptr, num_probes):
        """The caller rewrote these probes' blocks of the irradiance atlas itself: a tracked fp32 copy of it is patched (see sah_hip.h)."""
        self._check(self.lib.sah_probe_notify_updated(self.handle, C.byref(probe_irradiance), C.c_void_p(probes_ptr), num_probes))

    def shadow_render(self, scene, sun, num_cascades, shadowmap, stats_ptr=None):
        """scene: _abi.SceneGeometry of device addresses; stats_ptr: device address of 8 uint32 or None."""
        self._check(self.lib.sah_shadow_render(self.handle, C.byref(scene), C.byref(sun), num_cascades, C.byref(shadowmap), C.c_void_p(stats_ptr)))

    def gbuffer_render(self, scene, view, gbuffer, stats_ptr=None):
        self._check(self.lib.sah_gbuffer_render(self.handle, C.byref(scene), C.byref(view), C.byref(gbuffer), C.c_void_p(stats_ptr)))

    def motion_vectors_render(self, scene, view, depth, out, stats=None):
        """sah_motion_vectors_render (include/sah_motion_vectors.h): depth, out: _abi.Plane of device memory (D32_SFLOAT read only,
        R16G16_SFLOAT of the same extent); stats: device pointer to SAH_RASTER_STATS_WORDS words, or None."""
        self._check(self.lib.sah_motion_vectors_render(self.handle, C.byref(scene), C.byref(view), C.byref(depth), C.byref(out), C.c_void_p(stats)))

    def gbuffer_motion_render(self, scene, view, gbuffer, out, stats=None):
        """sah_gbuffer_motion_render (include/sah_gbuffer_motion.h): gbuffer_render into `gbuffer` (_abi.GBuffer) and motion_vectors_render
        against its depth plane into `out` (_abi.Plane, R16G16_SFLOAT of the same extent) with one rasteriser set-up; stats: device pointer to
        SAH_RASTER_STATS_WORDS words (the G-buffer pass's), or None."""
        self._check(self.lib.sah_gbuffer_motion_render(self.handle, C.byref(scene), C.byref(view), C.byref(gbuffer), C.byref(out), C.c_void_p(stats)))

    RASTER_PASS_FIELDS = ("attempts", "record_capacity", "clip_capacity", "pairs_capacity")

    def raster_last_pass(self):
        """Test hook (sah_debug_raster_last_pass): how the last shadow / G-buffer / RSM / motion-vectors call of this context sized its scratch,
        as a dict — attempts (2 or more: a buffer was too small and the pass was rendered again) and the record, clip-queue and bin-list
        capacities of the last attempt.  Recorded on the host: no device work, no synchronisation."""
        out = (C.c_uint32 * len(self.RASTER_PASS_FIELDS))()
        self._check(self.lib.sah_debug_raster_last_pass(self.handle, out))
        return {k: int(v) for k, v in zip(self.RASTER_PASS_FIELDS, out)}

    def vrsaa_measure_aliasing(self, color, depth, contrast, rows=(0, 0)):
        """sah_vrsaa_measure_aliasing (include/sah_vrsaa.h): color R8G8B8A8_SRGB, depth D32_SFLOAT, contrast R16G16_SFLOAT, _abi.Plane of device
        memory of one extent; rows of `contrast` to write, (0, 0) = all."""
        self._check(self.lib.sah_vrsaa_measure_aliasing(self.handle, C.byref(color), C.byref(depth), C.byref(contrast), rows[0], rows[1]))

    def taa_resolve(self, lit, depth, motion_vectors, history, out, params, rows=(0, 0)):
        """sah_taa_resolve (include/sah_taa.h): lit, history, out R16G16B16A16_SFLOAT, depth D32_SFLOAT, motion_vectors R16G16_SFLOAT, _abi.Plane
        of device memory, one extent; params an _abi.TaaParams.  history may be None with _abi.TAA_HISTORY_INVALID in params.flags.  rows
        (begin, end) of `out`, (0, 0) = all."""
        self._check(self.lib.sah_taa_resolve(self.handle, C.byref(lit), C.byref(depth), C.byref(motion_vectors), None if history is None else C.byref(history),
                                             C.byref(out), C.byref(params), rows[0], rows[1]))

    def taa_upscale(self, lit, depth, motion_vectors, history, out, params, rows=(0, 0)):
        """sah_taa_upscale (include/sah_taa_upscale.h): lit R16G16B16A16_SFLOAT, depth D32_SFLOAT, motion_vectors R16G16_SFLOAT of the render
        extent, history and out R16G16B16A16_SFLOAT of the output extent (no smaller), _abi.Plane of device memory; params an
        _abi.TaaUpscaleParams.  history may be None with _abi.TAA_HISTORY_INVALID in params.flags.  rows (begin, end) of `out`, (0, 0) = all."""
        self._check(self.lib.sah_taa_upscale(self.handle, C.byref(lit), C.byref(depth), C.byref(motion_vectors), None if history is None else C.byref(history),
                                             C.byref(out), C.byref(params), rows[0], rows[1]))

    def ssao(self, view_data, depth, normals, scratch, ao_out, params, rows=(0, 0)):
        """sah_ssao (include/sah_ssao.h): depth D32_SFLOAT, normals R16G16B16A16_SFLOAT, scratch and ao_out R32_SFLOAT, _abi.Plane of device
        memory, one extent; params an _abi.SsaoParams.  scratch may be None with params.blur_passes == 0.  rows (begin, end) of `ao_out`,
        (0, 0) = all."""
        self._check(self.lib.sah_ssao(self.handle, C.byref(view_data), C.byref(depth), C.byref(normals), None if scratch is None else C.byref(scratch),
                                      C.byref(ao_out), C.byref(params), rows[0], rows[1]))

    def rt_denoise(self, view_data, desc, params, rows=(0, 0)):
        """sah_rt_denoise (include/sah_rt_denoise.h): desc an _abi.RtDenoiseDesc (RtDenoiseDesc.of(noisy=..., ...), _abi.Plane of device
        memory, one extent), params an _abi.RtDenoiseParams.  previous_depth, history and history_length may be None with
        RT_DENOISE_HISTORY_INVALID in params.flags.  rows (begin, end) of `denoised`, (0, 0) = all."""
        self._check(self.lib.sah_rt_denoise(self.handle, C.byref(view_data), C.byref(desc), C.byref(params), rows[0], rows[1]))

    def rtgi_denoise(self, view_data, desc, params, rows=(0, 0)):
        """sah_rtgi_denoise (include/sah_rtgi_denoise.h): desc an _abi.RtgiDenoiseDesc (RtgiDenoiseDesc.of(ray_buffer=..., ...), _abi.Plane of
        device memory, one extent), params an _abi.RtgiDenoiseParams.  previous_depth, history and history_moments may be None with
        RTGI_DENOISE_HISTORY_INVALID in params.flags.  rows (begin, end) of the two denoised planes, (0, 0) = all."""
        self._check(self.lib.sah_rtgi_denoise(self.handle, C.byref(view_data), C.byref(desc), C.byref(params), rows[0], rows[1]))

    def exposure_meter(self, scene, state_in, state_out, work, exposed_out, params):
        """sah_exposure_meter (include/sah_exposure.h): scene and exposed_out R16G16B16A16_SFLOAT _abi.Plane of device memory, one extent;
        state_in, state_out (16 bytes each) and work (EXPOSURE_WORK_BYTES) device addresses; params an _abi.ExposureParams.  state_in may be
        None with _abi.EXPOSURE_HISTORY_INVALID in params.flags; exposed_out None = meter only, a plane = the fused form."""
        self._check(self.lib.sah_exposure_meter(self.handle, C.byref(scene), C.c_void_p(state_in), C.c_void_p(state_out), C.c_void_p(work),
                                                None if exposed_out is None else C.byref(exposed_out), C.byref(params)))

    def exposure_apply(self, scene, state, out, rows=(0, 0)):
        """sah_exposure_apply: out.rgb = scene.rgb * state->exposure; state a device address; out may be the plane `scene` itself.  rows
        (begin, end) of `out`, (0, 0) = all."""
        self._check(self.lib.sah_exposure_apply(self.handle, C.byref(scene), C.c_void_p(state), C.byref(out), rows[0], rows[1]))

    def sharpen(self, scene, exposure_state, out, params, rows=(0, 0)):
        """sah_sharpen (include/sah_sharpen.h): scene and out R16G16B16A16_SFLOAT _abi.Plane of device memory, one extent, not overlapping;
        exposure_state the device address of a 16-byte exposure state, or None; params an _abi.SharpenParams.  rows (begin, end) of `out`,
        (0, 0) = all."""
        self._check(self.lib.sah_sharpen(self.handle, C.byref(scene), C.c_void_p(exposure_state), C.byref(out), C.byref(params), rows[0], rows[1]))

    def ssr(self, view_data, color, normals, data, depth, source, lit, scratch, out, params, rows=(0, 0)):
        """sah_ssr (include/sah_ssr.h): color R8G8B8A8_SRGB, normals R16G16B16A16_SFLOAT, data R8G8B8A8_UNORM, depth D32_SFLOAT (the G-buffer's),
        source, lit and out R16G16B16A16_SFLOAT, one extent W x H; scratch R32_SFLOAT, ceil(W / 8) x ceil(H / 8); _abi.Plane of device memory.
        lit may be the plane `source`; out overlaps nothing.  params an _abi.SsrParams.  rows (begin, end) of `out`, (0, 0) = all."""
        self._check(self.lib.sah_ssr(self.handle, C.byref(view_data), C.byref(color), C.byref(normals), C.byref(data), C.byref(depth), C.byref(source),
                                     C.byref(lit), C.byref(scratch), C.byref(out), C.byref(params), rows[0], rows[1]))

    def motion_blur(self, scene, depth, motion_vectors, tiles, out, params, rows=(0, 0)):
        """sah_motion_blur (include/sah_motion_blur.h): scene and out R16G16B16A16_SFLOAT, W x H; depth D32_SFLOAT and motion_vectors
        R16G16_SFLOAT, w x h <= W x H; tiles R16G16_SFLOAT scratch, ceil(w / 16) x ceil(h / 16), written by the call; _abi.Plane of device
        memory.  out overlaps nothing, tiles no input.  params an _abi.MotionBlurParams.  rows (begin, end) of `out`, (0, 0) = all."""
        self._check(self.lib.sah_motion_blur(self.handle, C.byref(scene), C.byref(depth), C.byref(motion_vectors), C.byref(tiles), C.byref(out),
                                             C.byref(params), rows[0], rows[1]))

    def sun_shafts(self, view_data, sun, shadowmap, depth, lit, march, out, params, rows=(0, 0)):
        """sah_sun_shafts (include/sah_sun_shafts.h): view_data an _abi.ViewData, sun an _abi.SunLightConstants, shadowmap the _abi.Volume
        lighting() takes in CSM mode or None (every sample lit); depth D32_SFLOAT, lit and out R16G16B16A16_SFLOAT, w x h; march
        R16G16B16A16_SFLOAT scratch, ceil(w / s) x ceil(h / s), written by the call; _abi.Plane of device memory.  lit may be None under
        SUN_SHAFTS_TERM_ONLY.  params an _abi.SunShaftsParams.  rows (begin, end) of `out`, (0, 0) = all."""
        def ref(o):
            return None if o is None else C.byref(o)
        self._check(self.lib.sah_sun_shafts(self.handle, ref(view_data), ref(sun), ref(shadowmap), ref(depth), ref(lit), ref(march), ref(out),
                                            ref(params), rows[0], rows[1]))

    def translucent_render(self, desc, scene, stats_ptr=None):
        """sah_translucent_render (include/sah_translucent.h): desc the _abi.LightingDesc of the frame (its lit plane is blended into, its depth
        plane tested against), scene the _abi.SceneGeometry whose primitives of type PRIMITIVE_TYPE_TRANSLUCENT are drawn, back to front;
        stats_ptr: device pointer to SAH_RASTER_STATS_WORDS words, or None."""
        t = _abi.TranslucentDesc(C.pointer(desc), C.pointer(scene), C.c_void_p(stats_ptr))
        self._check(self.lib.sah_translucent_render(self.handle, C.byref(t)))

    def lighting_vrs(self, desc, sri, texel_size, depth_tolerance):
        """sah_lighting_vrs (include/sah_vrs.h): desc the _abi.LightingDesc lighting() takes, sri the R8_UINT shading-rate image (_abi.Plane of
        device memory), texel_size (x, y) pixels of `lit` per texel of it, depth_tolerance the relative depth difference up to which a pixel
        takes its coarse pixel's representative.  Every pixel gets the bytes lighting(desc) writes at its source pixel."""
        v = _abi.LightingVrsDesc(C.pointer(desc), C.pointer(sri), (C.c_uint32 * 2)(int(texel_size[0]), int(texel_size[1])), float(depth_tolerance))
        self._check(self.lib.sah_lighting_vrs(self.handle, C.byref(v)))

    def vrsaa_resolve(self, lit, out, rows=(0, 0)):
        """sah_vrsaa_resolve (include/sah_vrs.h): lit 2W x 2H, out W x H, R16G16B16A16_SFLOAT _abi.Plane of device memory; rows (begin, end) of
        `out`, (0, 0) = all."""
        self._check(self.lib.sah_vrsaa_resolve(self.handle, C.byref(lit), C.byref(out), rows[0], rows[1]))

    def vrsaa_shading_rate_image(self, contrast, sri, params):
        """sah_vrsaa_shading_rate_image: contrast R16G16_SFLOAT, sri R8_UINT (_abi.Plane of device memory), params an _abi.ShadingRateParams
        (scene.shading_rate_params)."""
        self._check(self.lib.sah_vrsaa_shading_rate_image(self.handle, C.byref(contrast), C.byref(sri), C.byref(params)))

    def mip_chain_generate(self, src, levels):
        """sah_mip_chain_generate (include/sah_mip_chain.h): src an _abi.Plane of device memory, levels a sequence of _abi.Plane, the levels
        of one image from level 0 on."""
        arr = (_abi.Plane * len(levels))(*levels)
        self._check(self.lib.sah_mip_chain_generate(self.handle, C.byref(src), arr, len(levels)))

    def rsm_render(self, scene, sun, cascades, num_cascades, rsm, stats_ptr=None):
        """cascades: (LpvCascadeMatrices * n) host array; rsm: _abi.RsmTargets of device volumes."""
        self._check(self.lib.sah_rsm_render(self.handle, C.byref(scene), C.byref(sun), cascades, num_cascades, C.byref(rsm), C.c_void_p(stats_ptr)))

    def lpv_extract_vpls(self, rsm, cascades, cascade_index, grid_cell_size, vpl_list_ptr, vpl_count_ptr):
        self._check(self.lib.sah_lpv_extract_vpls(self.handle, C.byref(rsm), cascades, cascade_index, grid_cell_size, C.c_void_p(vpl_list_ptr),
                                                  C.c_void_p(vpl_count_ptr)))

    def lpv_inject_vpls(self, vpl_list_ptr, vpl_count_ptr, capacity, cascades, cascade_index, num_cascades, rgb):
        vols = (_abi.Volume * 3)(*rgb)
        self._check(self.lib.sah_lpv_inject_vpls(self.handle, C.c_void_p(vpl_list_ptr), C.c_void_p(vpl_count_ptr), capacity, cascades, cascade_index,
                                                 num_cascades, vols))

    def rt_build(self, scene):
        """(Re)builds the context's acceleration structure over `scene` (_abi.SceneGeometry of device addresses, which must stay alive while
        rays are traced); returns [triangles kept, left out, levels, 0]."""
        stats = (C.c_uint32 * _abi.RT_STATS_WORDS)()
        self._check(self.lib.sah_rt_build(self.handle, C.byref(scene), stats))
        self._rt_scene = scene  # keeps the descriptor's arrays alive
        return list(stats)

    def rt_refit(self, scene, stats_ptr=None):
        """sah_rt_refit (include/sah_rt_refit.h): refreshes the structure of the last rt_build from `scene` (_abi.SceneGeometry of device
        addresses, same counts and topology; kept alive as rt_build keeps its scene) on the context's stream, without a host
        synchronisation.  stats_ptr: device address of 4 words (present, absent, bits of S, 0) or None."""
        self._check(self.lib.sah_rt_refit(self.handle, C.byref(scene), C.c_void_p(stats_ptr)))
        self._rt_scene = scene

    def rtao(self, view, depth, normals, noise, samples_per_pixel, max_ray_distance, ao_out):
        self._check(self.lib.sah_rtao(self.handle, C.byref(view), C.byref(depth), C.byref(normals), C.byref(noise), samples_per_pixel, max_ray_distance,
                                      C.byref(ao_out)))

    def sun_shadow_mask(self, view, sun, depth, normals, noise, mask_out):
        self._check(self.lib.sah_sun_shadow_mask(self.handle, C.byref(view), C.byref(sun), C.byref(depth), C.byref(normals), C.byref(noise), C.byref(mask_out)))

    def rt_set_rows(self, row_begin=0, row_end=0):
        """output rows [row_begin, row_end) for rtao / sun_shadow_mask / rtgi_trace from now on; (0, 0) = all"""
        self._check(self.lib.sah_rt_set_rows(self.handle, row_begin, row_end))

    def rt_set_bounces(self, num_bounces=0):
        """remaining_bounces of the rays probe_trace / rtgi_trace generate from now on (0..2; 0 = what the reference's generators set)"""
        self._check(self.lib.sah_rt_set_bounces(self.handle, num_bounces))

    def rt_structure(self):
        """Test hook (sah_debug_rt_structure): the structure the last rt_build left behind, read back to host memory (synchronises) — a dict
        of num_tris, num_levels, pad_bits (the fp32 pad's bits), level_offset (node groups) and level_count (nodes) of the existing levels,
        tris (num_tris records of RT_TRIANGLE, structure order) and nodes (node groups x {lo, hi} x axis x lane, float32)."""
        header = (C.c_uint32 * RT_STRUCTURE_HEADER_WORDS)()
        self._check(self.lib.sah_debug_rt_structure(self.handle, header, None, 0, None, 0))  # the sizes
        num_tris, num_levels, groups = int(header[0]), int(header[1]), int(header[2])
        tris, nodes = np.zeros(num_tris, RT_TRIANGLE), np.zeros((groups, 2, 3, 4), np.float32)
        self._check(self.lib.sah_debug_rt_structure(self.handle, header, tris.ctypes.data, tris.nbytes, nodes.ctypes.data, nodes.nbytes))
        assert (int(header[0]), int(header[1]), int(header[2])) == (num_tris, num_levels, groups)
        return {"num_tris": num_tris, "num_levels": num_levels, "pad_bits": int(header[3]),
                "level_offset": [int(v) for v in header[4:4 + num_levels]],
                "level_count": [int(v) for v in header[4 + RT_MAX_LEVELS:4 + RT_MAX_LEVELS + num_levels]],
                "header": [int(v) for v in header], "tris": tris, "nodes": nodes}

    def probe_trace(self, desc):
        """desc: _abi.ProbeTraceDesc (device addresses); 400 GI rays per probe into desc.trace_results."""
        self._check(self.lib.sah_probe_trace(self.handle, C.byref(desc)))

    def rtgi_trace(self, view, sun, sky, depth, normals, noise, ray_buffer, ray_irradiance):
        self._check(self.lib.sah_rtgi_trace(self.handle, C.byref(view), C.byref(sun), C.byref(sky), C.byref(depth), C.byref(normals), C.byref(noise),
                                            C.byref(ray_buffer), C.byref(ray_irradiance)))

    def allgather_rows(self, image, rows_per_rank, allocated_rows=None):
        """image: _abi.Plane over a buffer of `allocated_rows` (default image.height) rows; in place, on the context's stream."""
        self._check(self.lib.sah_allgather_rows(self.handle, C.byref(image), rows_per_rank, image.height if allocated_rows is None else allocated_rows))

    def allgather_rows_reversed(self, image, rows_per_rank, allocated_rows=None):
        self._check(self.lib.sah_allgather_rows_reversed(self.handle, C.byref(image), rows_per_rank,
                                                         image.height if allocated_rows is None else allocated_rows))

    def comm_set_stream(self, hip_stream_handle):
        self._check(self.lib.sah_comm_set_stream(self.handle, C.c_void_p(hip_stream_handle)))

    def comm_wait(self):
        self._check(self.lib.sah_comm_wait(self.handle))

    # ---- direct exchange (include/sah_hip.h): handles are plain bytes that the caller carries between the ranks
    def ipc_open(self):
        buf = C.create_string_buffer(_abi.IPC_HANDLE_BYTES)
        self._check(self.lib.sah_ipc_open(self.handle, buf))
        return buf.raw

    def ipc_connect(self, handles):
        """handles: every rank's ipc_open() result, in rank order"""
        self._check(self.lib.sah_ipc_connect(self.handle, C.create_string_buffer(b"".join(handles), len(handles) * _abi.IPC_HANDLE_BYTES)))

    def ipc_export(self, device_ptr, nbytes):
        buf = C.create_string_buffer(_abi.IPC_HANDLE_BYTES)
        self._check(self.lib.sah_ipc_export(self.handle, C.c_void_p(device_ptr), nbytes, buf))
        return buf.raw

    def ipc_register(self, device_ptr, nbytes, handles):
        self._check(self.lib.sah_ipc_register(self.handle, C.c_void_p(device_ptr), nbytes,
                                              C.create_string_buffer(b"".join(handles), len(handles) * _abi.IPC_HANDLE_BYTES)))

    def ipc_unregister(self, device_ptr):
        """Before a registered buffer is freed (every rank, same order): waits for the context's streams and frees the registration."""
        self._check(self.lib.sah_ipc_unregister(self.handle, C.c_void_p(device_ptr)))

    def ipc_reset(self):
        """After SahError COMM from the direct exchange, collectively: sync (ignore its error), barrier, ipc_reset, barrier (see sah_hip.h)."""
        self._check(self.lib.sah_ipc_reset(self.handle))

    def allgather_bytes(self, device_ptr, bytes_per_rank):
        self._check(self.lib.sah_allgather_bytes(self.handle, C.c_void_p(device_ptr), bytes_per_rank))

    # ---- the sharded frame as a loop of the library (sah_chain_*): handles are plain integers, androidrenderer_amd/chain.py wraps them
    def chain_create(self, plan, frames, tonemap_flags, chain_flags, work_stream, reduce_stream, post_stream):
        h = C.c_void_p()
        self._check(self.lib.sah_chain_create(self.handle, C.byref(plan), frames, tonemap_flags, chain_flags, C.c_void_p(work_stream),
                                              C.c_void_p(reduce_stream) if reduce_stream else None, C.c_void_p(post_stream) if post_stream else None, C.byref(h)))
        return h

    def chain_submit(self, chain, begin_event=None, end_event=None):
        self._check(self.lib.sah_chain_submit(chain, C.c_void_p(begin_event) if begin_event else None, C.c_void_p(end_event) if end_event else None))

    def chain_flush(self, chain):
        self._check(self.lib.sah_chain_flush(chain))

    def chain_graphs(self, chain):
        """(graph replays, captures, 1 if a capture failed and the chain fell back to direct calls)"""
        out = (C.c_uint64 * 3)()
        self._check(self.lib.sah_debug_chain_graphs(chain, out))
        if out[2]:
            print("[sah] " + self.lib.sah_last_error(self.handle).decode())
        return int(out[0]), int(out[1]), int(out[2])

    def chain_destroy(self, chain):
        self.lib.sah_chain_destroy(chain)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.sah_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    lib = load()
    buf = C.create_string_buffer(128)
    rc = lib.sah_comm_unique_id(buf)
    if rc != _abi.SAH_OK:
        raise SahError(rc, lib.sah_status_string(rc).decode())
    return buf.raw
