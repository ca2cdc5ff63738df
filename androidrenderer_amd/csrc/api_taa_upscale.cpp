// C ABI: temporal upscaling (include/sah_taa_upscale.h; kernel in taa_upscale.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_taa_upscale.h"
#include "ctx.hpp"
#include "launch.hpp"

extern "C" int sah_taa_upscale(sah_ctx* ctx, const sah_plane* lit, const sah_plane* depth, const sah_plane* motion_vectors, const sah_plane* history,
                               const sah_plane* out, const sah_taa_upscale_params* params, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_taa_upscale_params) == 28, "sah_taa_upscale_params is 28 bytes");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: params is null");
    if (params->flags & ~(SAH_TAA_HISTORY_INVALID | SAH_TAA_HDR_WEIGHTS)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: unknown flag bits");
    const bool use_history = !(params->flags & SAH_TAA_HISTORY_INVALID);
    const PlaneSpec planes[5] = {{lit, SAH_FORMAT_R16G16B16A16_SFLOAT, "lit (R16G16B16A16_SFLOAT)"},
                                 {depth, SAH_FORMAT_D32_SFLOAT, "depth (D32_SFLOAT)"},
                                 {motion_vectors, SAH_FORMAT_R16G16_SFLOAT, "motion_vectors (R16G16_SFLOAT)"},
                                 {out, SAH_FORMAT_R16G16B16A16_SFLOAT, "out (R16G16B16A16_SFLOAT)"},
                                 {history, SAH_FORMAT_R16G16B16A16_SFLOAT, "history (R16G16B16A16_SFLOAT; NULL only with SAH_TAA_HISTORY_INVALID)"}};
    const int num_planes = use_history ? 5 : 4;  // (a history that is not read is not looked at)
    if (const int rc = check_planes(ctx, "taa_upscale", planes, num_planes); rc != SAH_OK) return rc;
    const uint32_t w = lit->width, h = lit->height, W = out->width, H = out->height;
    for (int i = 1; i < 3; i++)
        if (planes[i].p->width != w || planes[i].p->height != h)
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: lit, depth and motion_vectors must have one extent (the render resolution)");
    if (use_history && (history->width != W || history->height != H))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: history and out must have one extent (the output resolution)");
    if (w > W || h > H) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: %u x %u to %u x %u is downscaling", w, h, W, H);
    if (texel_count_too_large(w, h) || texel_count_too_large(W, H)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: 2^32 texels or more");
    if (!resolve_rows(&row_begin, &row_end, H)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: bad row range");
    if (!(params->blend > 0.0f && params->blend <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: blend must be in (0, 1]");
    if (!(params->min_confidence >= 0.0f && params->min_confidence <= 1.0f))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: min_confidence must be in [0, 1]");
    for (const float j : {params->jitter[0], params->jitter[1], params->previous_jitter[0], params->previous_jitter[1]})
        if (!std::isfinite(j)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: a jitter is not finite");
    for (int i = 0; i < num_planes; i++)
        if (i != 3 && overlaps(byte_range(out), byte_range(planes[i].p)))
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: out overlaps an input (the pass gathers from a neighbourhood: not in place)");
    sah::TaaUpscaleArgs a{};
    a.lit = parg(lit), a.depth = parg(depth), a.mv = parg(motion_vectors), a.out = parg(out);
    a.history = use_history ? parg(history) : sah::PlaneArg{nullptr, 0};
    a.w = w, a.h = h, a.W = W, a.H = H, a.row_begin = row_begin, a.row_end = row_end;
    a.blend = params->blend, a.min_confidence = params->min_confidence;
    a.jx = params->jitter[0], a.jy = params->jitter[1];
    a.djx = params->previous_jitter[0] - params->jitter[0];
    a.djy = params->previous_jitter[1] - params->jitter[1];
    a.sx = (float)w / (float)W, a.sy = (float)h / (float)H;
    a.rx = (float)W / (float)w, a.ry = (float)H / (float)h;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_taa_upscale(a, use_history, (params->flags & SAH_TAA_HDR_WEIGHTS) != 0, ctx->stream));
    return SAH_OK;
}
