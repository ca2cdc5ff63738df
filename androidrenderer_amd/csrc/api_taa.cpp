// C ABI: temporal anti-aliasing (include/sah_taa.h; kernel in taa.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_taa.h"
#include "ctx.hpp"
#include "launch.hpp"

extern "C" int sah_taa_resolve(sah_ctx* ctx, const sah_plane* lit, const sah_plane* depth, const sah_plane* motion_vectors, const sah_plane* history,
                               const sah_plane* out, const sah_taa_params* params, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_taa_params) == 24, "sah_taa_params is 24 bytes");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_resolve: params is null");
    if (params->flags & ~(SAH_TAA_HISTORY_INVALID | SAH_TAA_HDR_WEIGHTS)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_resolve: unknown flag bits");
    const bool use_history = !(params->flags & SAH_TAA_HISTORY_INVALID);
    const PlaneSpec planes[5] = {{lit, SAH_FORMAT_R16G16B16A16_SFLOAT, "lit (R16G16B16A16_SFLOAT)"},
                                 {depth, SAH_FORMAT_D32_SFLOAT, "depth (D32_SFLOAT)"},
                                 {motion_vectors, SAH_FORMAT_R16G16_SFLOAT, "motion_vectors (R16G16_SFLOAT)"},
                                 {out, SAH_FORMAT_R16G16B16A16_SFLOAT, "out (R16G16B16A16_SFLOAT)"},
                                 {history, SAH_FORMAT_R16G16B16A16_SFLOAT, "history (R16G16B16A16_SFLOAT; NULL only with SAH_TAA_HISTORY_INVALID)"}};
    const int num_planes = use_history ? 5 : 4;  // (a history that is not read is not looked at)
    if (const int rc = check_planes(ctx, "taa_resolve", planes, num_planes); rc != SAH_OK) return rc;
    const uint32_t w = out->width, h = out->height;
    for (int i = 0; i < num_planes; i++)
        if (planes[i].p->width != w || planes[i].p->height != h) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_resolve: the planes must have one extent");
    if (texel_count_too_large(w, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_resolve: 2^32 texels or more");
    if (!resolve_rows(&row_begin, &row_end, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_resolve: bad row range");
    if (!(params->blend > 0.0f && params->blend <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_resolve: blend must be in (0, 1]");
    for (const float j : {params->jitter[0], params->jitter[1], params->previous_jitter[0], params->previous_jitter[1]})
        if (!std::isfinite(j)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_resolve: a jitter is not finite");
    for (int i = 0; i < num_planes; i++)
        if (i != 3 && overlaps(byte_range(out), byte_range(planes[i].p)))
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_resolve: out overlaps an input (the pass reads a 3 x 3 neighbourhood: not in place)");
    sah::TaaArgs a{};
    a.lit = parg(lit), a.depth = parg(depth), a.mv = parg(motion_vectors), a.out = parg(out);
    a.history = use_history ? parg(history) : sah::PlaneArg{nullptr, 0};
    a.W = w, a.H = h, a.row_begin = row_begin, a.row_end = row_end;
    a.blend = params->blend;
    a.djx = params->previous_jitter[0] - params->jitter[0];
    a.djy = params->previous_jitter[1] - params->jitter[1];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_taa_resolve(a, use_history, (params->flags & SAH_TAA_HDR_WEIGHTS) != 0, ctx->stream));
    return SAH_OK;
}
