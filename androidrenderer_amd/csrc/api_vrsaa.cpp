// C ABI: the two VRSAA passes (include/sah_vrsaa.h; kernels in vrsaa.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_vrsaa.h"
#include "ctx.hpp"
#include "launch.hpp"

extern "C" {

int sah_vrsaa_measure_aliasing(sah_ctx* ctx, const sah_plane* scene_color, const sah_plane* depth, const sah_plane* contrast, uint32_t row_begin,
                               uint32_t row_end) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    const PlaneSpec planes[3] = {{scene_color, SAH_FORMAT_R8G8B8A8_SRGB, "scene_color (R8G8B8A8_SRGB)"},
                                 {depth, SAH_FORMAT_D32_SFLOAT, "depth (D32_SFLOAT)"},
                                 {contrast, SAH_FORMAT_R16G16_SFLOAT, "contrast (R16G16_SFLOAT)"}};
    if (const int rc = check_planes(ctx, "measure_aliasing", planes, 3); rc != SAH_OK) return rc;
    const uint32_t w = contrast->width, h = contrast->height;
    if (scene_color->width != w || scene_color->height != h || depth->width != w || depth->height != h)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "measure_aliasing: the three planes must have one extent");
    // (not texel_count_too_large: this entry has always taken an extent of 2^31 and more as long as the product fits)
    if ((uint64_t)w * h >= (1ull << 32)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "measure_aliasing: 2^32 texels or more");
    if (!resolve_rows(&row_begin, &row_end, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "measure_aliasing: bad row range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_vrsaa_contrast(parg(scene_color), parg(depth), parg(contrast), w, h, row_begin, row_end, ctx->luts, ctx->stream));
    return SAH_OK;
}

int sah_vrsaa_shading_rate_image(sah_ctx* ctx, const sah_plane* contrast, const sah_plane* shading_rate_image, const sah_shading_rate_params* params) {
    SAH_RANGE();
    static_assert(sizeof(sah_shading_rate_params) == 92, "ShadingRateParams is 92 bytes (sampling_rate_calculator.cpp:126-132)");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "shading_rate_image: params is null");
    if (const int rc = plane_status(contrast, SAH_FORMAT_R16G16_SFLOAT); rc != SAH_OK)
        return fail(ctx, rc, "shading_rate_image: contrast must be an R16G16_SFLOAT plane, 4-byte aligned, with a pitch of at least a row");
    const sah_plane* s = shading_rate_image;
    if (!s || !s->ptr) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "shading_rate_image: no target");
    if (s->format != SAH_FORMAT_R8_UINT) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "shading_rate_image: the target must be an R8_UINT plane");
    if (!s->width || !s->height || s->row_pitch_bytes < s->width) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "shading_rate_image: bad target extent or pitch");
    if (params->contrast_image_resolution[0] != contrast->width || params->contrast_image_resolution[1] != contrast->height ||
        params->shading_rate_image_resolution[0] != s->width || params->shading_rate_image_resolution[1] != s->height)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "shading_rate_image: the resolutions in params are not the planes' extents");
    if (params->num_shading_rates > 8) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "shading_rate_image: more than 8 shading rates");
    // generate_shading_rate_image.comp:26 — float(uvec2) takes .x; ties to even (the host's default rounding mode, as v_rndne_f32)
    const float ratio = std::nearbyint((float)contrast->width / (float)s->width);
    const uint64_t d = ratio < 1.0f ? 1u : (uint64_t)ratio;
    if (d * s->width >= (1ull << 31) || d * s->height >= (1ull << 31) || (uint64_t)contrast->width * contrast->height >= (1ull << 32))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "shading_rate_image: extents too large (block coordinates of 2^31 or more)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_vrsaa_shading_rate(parg(contrast), contrast->width, contrast->height, parg(s), s->width, s->height, (uint32_t)d, *params, ctx->stream));
    return SAH_OK;
}

}  // extern "C"
