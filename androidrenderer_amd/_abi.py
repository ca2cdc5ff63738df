"""ctypes mirror of include/sah_hip.h (the C ABI). Field order and sizes must match the header exactly;
tests/test_abi.py checks the struct sizes against the values the library reports."""
import ctypes as C

SAH_OK = 0
SAH_ERR_INVALID_ARGUMENT = -1
SAH_ERR_UNSUPPORTED_FORMAT = -2
SAH_ERR_HIP = -3
SAH_ERR_NO_DEVICE = -4
SAH_ERR_COMM = -5
SAH_ERR_UNSUPPORTED = -6

FORMAT_R8_UNORM = 9
FORMAT_R8G8B8A8_UNORM = 37
FORMAT_R8G8B8A8_SRGB = 43
FORMAT_R16_SFLOAT = 76
FORMAT_R16G16_SFLOAT = 83
FORMAT_R16G16B16A16_SFLOAT = 97
FORMAT_R32_SFLOAT = 100
FORMAT_B10G11R11_UFLOAT_PACK32 = 122
FORMAT_D16_UNORM = 124
FORMAT_D32_SFLOAT = 126
FORMAT_R8_UINT = 13  # include/sah_vrsaa.h: accepted by the VRSAA entries only

FORMAT_BPP = {9: 1, 13: 1, 37: 4, 43: 4, 76: 2, 83: 4, 97: 8, 100: 4, 122: 4, 124: 2, 126: 4}

SHADOW_MODE_OFF, SHADOW_MODE_CSM, SHADOW_MODE_RT = 0, 1, 2
GI_NONE, GI_LPV, GI_CACHE, GI_RTGI = 0, 1, 2, 3
LIGHTING_QUIRK_SUN_BLEND = 1 << 0
LIGHTING_BRUTE_FORCE_LIGHTS = 1 << 1
LIGHTING_DEFAULT_FLAGS = LIGHTING_QUIRK_SUN_BLEND
MAX_BLOOM_MIPS = 8
TONEMAP_TOLERANCE_1CODE = 1 << 0
# sah_debug_set's `strays` (a test hook, not in sah_hip.h): who shades the pixels the fast Lighting kernel lists — the context's record of recent
# calls decides, always the fix-up launch, always the fast kernel itself.  Word 12 of sah_debug_lighting_dispatch reports 1 + (in-kernel) for a fast call.
DEBUG_STRAYS_AUTO, DEBUG_STRAYS_LAUNCH, DEBUG_STRAYS_INLINE = 0, 1, 2
GENERATION_TRACKED = 0xFFFFFFFF  # sah_gi::lpv_generation / probe_generation: the context keeps its gather copies current itself


class Plane(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("row_pitch_bytes", C.c_uint32),
                ("format", C.c_uint32)]


class Volume(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("depth", C.c_uint32),
                ("row_pitch_bytes", C.c_uint32), ("slice_pitch_bytes", C.c_uint32), ("format", C.c_uint32)]


TAA_HISTORY_INVALID, TAA_HDR_WEIGHTS = 1, 2  # SAH_TAA_* (include/sah_taa.h)


class TaaParams(C.Structure):  # sah_taa_params (include/sah_taa.h): 24 bytes
    _fields_ = [("blend", C.c_float), ("jitter", C.c_float * 2), ("previous_jitter", C.c_float * 2), ("flags", C.c_uint32)]


class SsaoParams(C.Structure):  # sah_ssao_params (include/sah_ssao.h): 40 bytes; default() = the reference's CACAO settings
    _fields_ = [("radius", C.c_float), ("max_radius_pixels", C.c_float), ("shadow_multiplier", C.c_float), ("shadow_clamp", C.c_float),
                ("horizon_angle_threshold", C.c_float), ("fade_out_from", C.c_float), ("fade_out_to", C.c_float), ("edge_sharpness", C.c_float),
                ("blur_passes", C.c_uint32), ("flags", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        values = dict(radius=8.0, max_radius_pixels=32.0, shadow_multiplier=1.0, shadow_clamp=0.98, horizon_angle_threshold=0.06, fade_out_from=50.0,
                      fade_out_to=300.0, edge_sharpness=50.0, blur_passes=2, flags=0)
        values.update(changes)
        return cls(**values)


EXPOSURE_HISTORY_INVALID = 1  # SAH_EXPOSURE_HISTORY_INVALID (include/sah_exposure.h)


class ExposureParams(C.Structure):  # sah_exposure_params (include/sah_exposure.h): 32 bytes; default() = the header's defaults
    _fields_ = [("key", C.c_float), ("low_fraction", C.c_float), ("high_fraction", C.c_float), ("min_exposure", C.c_float), ("max_exposure", C.c_float),
                ("adaptation", C.c_float), ("max_workgroups", C.c_uint32), ("flags", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        values = dict(key=0.18, low_fraction=0.5, high_fraction=0.95, min_exposure=1.0 / 64.0, max_exposure=64.0, adaptation=1.0, max_workgroups=0, flags=0)
        values.update(changes)
        return cls(**values)


class ExposureState(C.Structure):  # sah_exposure_state: 16 bytes of device memory
    _fields_ = [("exposure", C.c_float), ("adapted", C.c_float), ("metered", C.c_uint32), ("window", C.c_uint32)]


SHARPEN_DENOISE = 1  # SAH_SHARPEN_DENOISE (include/sah_sharpen.h)


class SharpenParams(C.Structure):  # sah_sharpen_params (include/sah_sharpen.h): 12 bytes
    _fields_ = [("sharpness", C.c_float), ("pre_scale", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def default(cls, **settings):
        values = dict(sharpness=1.0, pre_scale=1.0, flags=0)
        values.update(settings)
        return cls(**values)


SSR_JITTER, SSR_REFLECTION_ONLY = 1, 2  # SAH_SSR_* (include/sah_ssr.h)


class SsrParams(C.Structure):  # sah_ssr_params (include/sah_ssr.h): 36 bytes; default() = the header's defaults
    _fields_ = [("max_distance", C.c_float), ("thickness", C.c_float), ("stride_pixels", C.c_float), ("max_steps", C.c_uint32), ("refine_steps", C.c_uint32),
                ("max_roughness", C.c_float), ("edge_fade", C.c_float), ("intensity", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        values = dict(max_distance=50.0, thickness=0.5, stride_pixels=4.0, max_steps=64, refine_steps=4, max_roughness=0.6, edge_fade=0.1, intensity=1.0,
                      flags=0)
        values.update(changes)
        return cls(**values)


MOTION_BLUR_DITHER = 1  # SAH_MOTION_BLUR_DITHER (include/sah_motion_blur.h)


class MotionBlurParams(C.Structure):  # sah_motion_blur_params (include/sah_motion_blur.h): 44 bytes; default() = the header's defaults
    _fields_ = [("shutter", C.c_float), ("max_blur_pixels", C.c_float), ("min_velocity_pixels", C.c_float), ("sample_count", C.c_uint32),
                ("depth_extent", C.c_float), ("z_near", C.c_float), ("jitter", C.c_float * 2), ("previous_jitter", C.c_float * 2), ("flags", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        values = dict(shutter=0.5, max_blur_pixels=32.0, min_velocity_pixels=0.5, sample_count=12, depth_extent=1.0, z_near=0.1, jitter=(0.0, 0.0),
                      previous_jitter=(0.0, 0.0), flags=0)
        values.update(changes)
        for k in ("jitter", "previous_jitter"):
            values[k] = (C.c_float * 2)(*values[k])
        return cls(**values)


SUN_SHAFTS_DITHER, SUN_SHAFTS_TERM_ONLY = 1, 2  # SAH_SUN_SHAFTS_* (include/sah_sun_shafts.h)
LIGHTING_EXPOSURE = 0.00031415927  # the constant sah_lighting scales the sun's colour by (directional_light.frag)


class SunShaftsParams(C.Structure):  # sah_sun_shafts_params (include/sah_sun_shafts.h): 60 bytes; default() = the header's defaults
    _fields_ = [("step_length", C.c_float), ("num_steps", C.c_uint32), ("step_transmittance", C.c_float), ("albedo", C.c_float * 3),
                ("ambient", C.c_float * 3), ("anisotropy", C.c_float), ("depth_bias", C.c_float), ("depth_sharpness", C.c_float),
                ("downscale", C.c_uint32), ("dither_offset", C.c_uint32), ("flags", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        values = dict(step_length=0.5, num_steps=32, step_transmittance=0.98, albedo=(1.0, 1.0, 1.0), ambient=(0.0, 0.0, 0.0), anisotropy=0.6,
                      depth_bias=0.0005, depth_sharpness=50.0, downscale=1, dither_offset=0, flags=0)
        values.update(changes)
        for k in ("albedo", "ambient"):
            values[k] = (C.c_float * 3)(*values[k])
        return cls(**values)


RT_DENOISE_HISTORY_INVALID = 1  # SAH_RT_DENOISE_HISTORY_INVALID


class RtDenoiseParams(C.Structure):  # sah_rt_denoise_params (include/sah_rt_denoise.h): 40 bytes; default() = the header's defaults
    _fields_ = [("max_history", C.c_float), ("depth_tolerance", C.c_float), ("depth_sharpness", C.c_float), ("normal_squarings", C.c_uint32),
                ("passes", C.c_uint32), ("jitter", C.c_float * 2), ("previous_jitter", C.c_float * 2), ("flags", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        values = dict(max_history=32.0, depth_tolerance=0.1, depth_sharpness=50.0, normal_squarings=5, passes=3, jitter=(0.0, 0.0),
                      previous_jitter=(0.0, 0.0), flags=0)
        values.update(changes)
        for k in ("jitter", "previous_jitter"):
            values[k] = (C.c_float * 2)(*values[k])
        return cls(**values)


class RtDenoiseDesc(C.Structure):  # sah_rt_denoise_desc: ten plane pointers; of() keeps the planes alive with the descriptor
    PLANES = ("noisy", "depth", "normals", "motion_vectors", "previous_depth", "history", "history_length", "accum_out", "length_out", "denoised")
    _fields_ = [(name, C.POINTER(Plane)) for name in PLANES]

    @classmethod
    def of(cls, **planes):
        """planes by field name, each an _abi.Plane or None (NULL)"""
        unknown = set(planes) - set(cls.PLANES)
        if unknown:
            raise TypeError(f"not planes of sah_rt_denoise_desc: {sorted(unknown)}")
        self = cls()
        self._planes = dict(planes)
        for name, p in planes.items():
            if p is not None:
                setattr(self, name, C.pointer(p))
        return self


RTGI_DENOISE_HISTORY_INVALID = 1  # SAH_RTGI_DENOISE_HISTORY_INVALID
FORMAT_R32G32_SFLOAT = 103        # include/sah_rtgi_denoise.h: accepted by sah_rtgi_denoise only
FORMAT_R32G32B32A32_SFLOAT = 109
FORMAT_BPP.update({FORMAT_R32G32_SFLOAT: 8, FORMAT_R32G32B32A32_SFLOAT: 16})


class RtgiDenoiseParams(C.Structure):  # sah_rtgi_denoise_params (include/sah_rtgi_denoise.h): 52 bytes; default() = the header's defaults
    _fields_ = [("max_history", C.c_float), ("min_history", C.c_float), ("depth_tolerance", C.c_float), ("depth_sharpness", C.c_float),
                ("normal_squarings", C.c_uint32), ("passes", C.c_uint32), ("luminance_sigma", C.c_float), ("luminance_floor", C.c_float),
                ("jitter", C.c_float * 2), ("previous_jitter", C.c_float * 2), ("flags", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        values = dict(max_history=32.0, min_history=4.0, depth_tolerance=0.1, depth_sharpness=50.0, normal_squarings=5, passes=3, luminance_sigma=4.0,
                      luminance_floor=1e-6, jitter=(0.0, 0.0), previous_jitter=(0.0, 0.0), flags=0)
        values.update(changes)
        for k in ("jitter", "previous_jitter"):
            values[k] = (C.c_float * 2)(*values[k])
        return cls(**values)


class RtgiDenoiseDesc(C.Structure):  # sah_rtgi_denoise_desc: twelve plane pointers; of() keeps the planes alive with the descriptor
    PLANES = ("ray_buffer", "ray_irradiance", "depth", "normals", "motion_vectors", "previous_depth", "history", "history_moments", "accum_out",
              "moments_out", "denoised_ray_buffer", "denoised_irradiance")
    _fields_ = [(name, C.POINTER(Plane)) for name in PLANES]

    @classmethod
    def of(cls, **planes):
        """planes by field name, each an _abi.Plane or None (NULL)"""
        unknown = set(planes) - set(cls.PLANES)
        if unknown:
            raise TypeError(f"not planes of sah_rtgi_denoise_desc: {sorted(unknown)}")
        self = cls()
        self._planes = dict(planes)
        for name, p in planes.items():
            if p is not None:
                setattr(self, name, C.pointer(p))
        return self


class TaaUpscaleParams(C.Structure):  # sah_taa_upscale_params (include/sah_taa_upscale.h): 28 bytes; flags are the TAA_* bits
    _fields_ = [("blend", C.c_float), ("min_confidence", C.c_float), ("jitter", C.c_float * 2), ("previous_jitter", C.c_float * 2), ("flags", C.c_uint32)]


class ShadingRateParams(C.Structure):  # sah_shading_rate_params (include/sah_vrsaa.h): 92 bytes
    _fields_ = [("contrast_image_resolution", C.c_uint32 * 2), ("shading_rate_image_resolution", C.c_uint32 * 2), ("max_rate", C.c_uint32 * 2),
                ("num_shading_rates", C.c_uint32), ("rates", (C.c_uint32 * 2) * 8)]


class ProbeAtlases(C.Structure):  # sah_probe_atlases
    _fields_ = [("rtgi", Volume), ("light_cache", Volume), ("depth", Volume), ("average", Volume), ("validity", Volume)]


PRIMITIVE_TYPE_SOLID, PRIMITIVE_TYPE_CUTOUT = 0, 1
PRIMITIVE_TYPE_TRANSLUCENT = 2  # SAH_PRIMITIVE_TYPE_TRANSLUCENT (include/sah_translucent.h): drawn by sah_translucent_render only
RASTER_STATS_WORDS = 8
RT_STATS_WORDS = 4
IPC_HANDLE_BYTES = 128


class VertexData(C.Structure):  # sah_vertex_data, 40 bytes
    _fields_ = [("normal", C.c_float * 3), ("tangent", C.c_float * 4), ("texcoord", C.c_float * 2), ("color", C.c_uint32)]


class Material(C.Structure):  # sah_material, 112 bytes
    _fields_ = [("base_color_tint", C.c_float * 4), ("emission_factor", C.c_float * 4), ("metalness_factor", C.c_float),
                ("roughness_factor", C.c_float), ("opacity_threshold", C.c_float), ("padding1", C.c_float),
                ("base_color_texel", C.c_float * 4), ("normal_texel", C.c_float * 4), ("data_texel", C.c_float * 4),
                ("emission_texel", C.c_float * 4)]


class Primitive(C.Structure):  # sah_primitive, 96 bytes
    _fields_ = [("model", C.c_float * 16), ("first_index", C.c_uint32), ("index_count", C.c_uint32), ("vertex_offset", C.c_int32),
                ("type", C.c_uint32), ("material", C.c_uint32), ("padding", C.c_uint32 * 3)]


FILTER_NEAREST, FILTER_LINEAR = 0, 1
ADDRESS_REPEAT, ADDRESS_MIRRORED_REPEAT, ADDRESS_CLAMP_TO_EDGE = 0, 1, 2
MAX_TEXTURE_MIPS = 14
TEXTURE_NONE = 0xFFFFFFFF


class Sampler(C.Structure):  # sah_sampler, 40 bytes
    _fields_ = [("mag_filter", C.c_uint32), ("min_filter", C.c_uint32), ("mipmap_mode", C.c_uint32), ("address_u", C.c_uint32),
                ("address_v", C.c_uint32), ("mip_lod_bias", C.c_float), ("min_lod", C.c_float), ("max_lod", C.c_float),
                ("max_anisotropy", C.c_float), ("reserved", C.c_uint32)]


class Texture(C.Structure):  # sah_texture, 384 bytes
    _fields_ = [("mips", Plane * MAX_TEXTURE_MIPS), ("num_mips", C.c_uint32), ("padding", C.c_uint32), ("sampler", Sampler)]


class MaterialTextures(C.Structure):  # sah_material_textures, 16 bytes
    _fields_ = [("base_color", C.c_uint32), ("normal", C.c_uint32), ("data", C.c_uint32), ("emission", C.c_uint32)]


class SceneGeometry(C.Structure):  # sah_scene_geometry
    _fields_ = [("vertex_positions", C.c_void_p), ("vertex_data", C.c_void_p), ("indices", C.c_void_p), ("primitives", C.c_void_p),
                ("materials", C.c_void_p), ("num_vertices", C.c_uint32), ("num_indices", C.c_uint32), ("num_primitives", C.c_uint32),
                ("num_materials", C.c_uint32), ("textures", C.c_void_p), ("material_textures", C.c_void_p), ("num_textures", C.c_uint32),
                ("padding", C.c_uint32)]


class RsmTargets(C.Structure):  # sah_rsm_targets
    _fields_ = [("flux", Volume), ("normals", Volume), ("depth", Volume)]


class GBuffer(C.Structure):
    _fields_ = [("color", Plane), ("normals", Plane), ("data", Plane), ("emission", Plane), ("depth", Plane)]


class MipChain(C.Structure):
    _fields_ = [("mips", Plane * MAX_BLOOM_MIPS), ("num_mips", C.c_uint32)]


class ViewData(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("projection", C.c_float * 16), ("inverse_view", C.c_float * 16),
                ("inverse_projection", C.c_float * 16), ("last_frame_view", C.c_float * 16),
                ("last_frame_projection", C.c_float * 16), ("frustum", C.c_float * 4), ("z_near", C.c_float),
                ("material_texture_mip_bias", C.c_float), ("render_resolution", C.c_float * 2), ("jitter", C.c_float * 2),
                ("previous_jitter", C.c_float * 2)]


class SunLightConstants(C.Structure):
    _fields_ = [("direction_and_tan_size", C.c_float * 4), ("color", C.c_float * 4), ("csm_resolution", C.c_uint32 * 4),
                ("data", (C.c_float * 4) * 4), ("cascade_matrices", (C.c_float * 16) * 4),
                ("cascade_inverse_matrices", (C.c_float * 16) * 4), ("shadow_mode", C.c_uint32),
                ("num_shadow_samples", C.c_float), ("padding1", C.c_uint32), ("padding2", C.c_uint32)]


class LpvCascadeMatrices(C.Structure):
    _fields_ = [("rsm_vp", C.c_float * 16), ("inverse_rsm_vp", C.c_float * 16), ("world_to_cascade", C.c_float * 16),
                ("cascade_to_world", C.c_float * 16)]


class ProbeCascade(C.Structure):
    _fields_ = [("min", C.c_float * 3), ("probe_spacing", C.c_float)]


class GI(C.Structure):
    _fields_ = [("kind", C.c_uint32),
                ("lpv_red", Volume), ("lpv_green", Volume), ("lpv_blue", Volume),
                ("lpv_cascades", C.POINTER(LpvCascadeMatrices)), ("lpv_num_cascades", C.c_uint32), ("lpv_exposure", C.c_float),
                ("probe_irradiance", Volume), ("probe_depth", Volume), ("probe_validity", Volume),
                ("probe_cascades", ProbeCascade * 4), ("probe_size", C.c_uint32 * 2), ("cache_debug_mode", C.c_uint32),
                ("ray_buffer", Plane), ("ray_irradiance", Plane), ("noise", Plane), ("num_extra_rays", C.c_uint32),
                ("extra_ray_radius", C.c_float), ("lpv_generation", C.c_uint32), ("probe_generation", C.c_uint32)]


class SkyLuts(C.Structure):
    _fields_ = [("transmittance", Plane), ("sky_view", Plane)]


class PointLight(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("radius", C.c_float), ("color", C.c_float * 3), ("intensity", C.c_float)]


class LightList(C.Structure):
    _fields_ = [("lights", C.c_void_p), ("count", C.c_uint32)]


class LightingDesc(C.Structure):
    _fields_ = [("gbuffer", C.POINTER(GBuffer)), ("ao", C.POINTER(Plane)), ("lit", C.POINTER(Plane)),
                ("view", C.POINTER(ViewData)), ("sun", C.POINTER(SunLightConstants)), ("shadowmap", C.POINTER(Volume)),
                ("shadow_mask", C.POINTER(Plane)), ("lights", C.POINTER(LightList)), ("gi", C.POINTER(GI)),
                ("sky", C.POINTER(SkyLuts)), ("flags", C.c_uint32), ("row_begin", C.c_uint32), ("row_end", C.c_uint32)]


class LightingVrsDesc(C.Structure):  # sah_lighting_vrs_desc (include/sah_vrs.h)
    _fields_ = [("lighting", C.POINTER(LightingDesc)), ("shading_rate_image", C.POINTER(Plane)), ("texel_size", C.c_uint32 * 2),
                ("depth_tolerance", C.c_float)]


class TranslucentDesc(C.Structure):  # sah_translucent_desc (include/sah_translucent.h)
    _fields_ = [("lighting", C.POINTER(LightingDesc)), ("scene", C.POINTER(SceneGeometry)), ("stats", C.c_void_p)]


class ChainPlan(C.Structure):  # sah_chain_plan
    _fields_ = [("aa_rows", C.c_uint32 * 2), ("mip0_rows", C.c_uint32 * 2), ("mip1_rows", C.c_uint32 * 2), ("out_rows", C.c_uint32 * 2),
                ("mip1_rows_per_rank", C.c_uint32), ("mip1_allocated_rows", C.c_uint32), ("rows_per_rank", C.c_uint32),
                ("out_allocated_rows", C.c_uint32)]


class ChainFrame(C.Structure):  # sah_chain_frame
    _fields_ = [("lighting", C.POINTER(LightingDesc) * 2), ("lit", Plane), ("antialiased", Plane), ("bloom", MipChain), ("out", Plane)]


CHAIN_NO_EXCHANGE = 1 << 0
CHAIN_CAPTURE = 1 << 1

assert C.sizeof(ViewData) == 432
assert C.sizeof(SunLightConstants) == 640
assert C.sizeof(LpvCascadeMatrices) == 256
assert C.sizeof(ProbeCascade) == 16
assert C.sizeof(PointLight) == 32


class ProbeTraceDesc(C.Structure):  # sah_probe_trace_desc
    _fields_ = [("cascades", ProbeCascade * 4), ("probes_to_update", C.c_void_p), ("num_probes", C.c_uint32),
                ("sun", C.POINTER(SunLightConstants)), ("sky", C.POINTER(SkyLuts)), ("noise", C.POINTER(Plane)),
                ("probe_irradiance", Volume), ("probe_depth", Volume), ("probe_validity", Volume), ("probe_size", C.c_uint32 * 2),
                ("trace_results", Volume)]
