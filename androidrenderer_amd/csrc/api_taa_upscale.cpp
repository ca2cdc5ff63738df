// C ABI: temporal upscaling (include/sah_taa_upscale.h; kernel in taa_upscale.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_taa_upscale.h"
#include "ctx.hpp"
#include "launch.hpp"

namespace {
// 0, or the status a plane of `format` with `bpp`-byte texels earns (the alignment rules of sah_vrsaa_measure_aliasing)
int plane_status(const sah_plane* p, uint32_t format, uint32_t bpp) {
    if (!p || !p->ptr) return SAH_ERR_INVALID_ARGUMENT;
    if (p->format != format) return SAH_ERR_UNSUPPORTED_FORMAT;
    if (!p->width || !p->height || (uint64_t)p->row_pitch_bytes < (uint64_t)p->width * bpp || ((uintptr_t)p->ptr % 4) || (p->row_pitch_bytes % 4))
        return SAH_ERR_INVALID_ARGUMENT;
    return SAH_OK;
}
bool overlap(const sah_plane* a, uint32_t a_bpp, const sah_plane* b, uint32_t b_bpp) {
    const uintptr_t a0 = (uintptr_t)a->ptr, a1 = a0 + (uint64_t)(a->height - 1) * a->row_pitch_bytes + (uint64_t)a->width * a_bpp;
    const uintptr_t b0 = (uintptr_t)b->ptr, b1 = b0 + (uint64_t)(b->height - 1) * b->row_pitch_bytes + (uint64_t)b->width * b_bpp;
    return a0 < b1 && b0 < a1;
}
bool too_large(uint32_t w, uint32_t h) { return ((w | h) >> 31) || (uint64_t)w * h >= (1ull << 32); }
}  // namespace

extern "C" int sah_taa_upscale(sah_ctx* ctx, const sah_plane* lit, const sah_plane* depth, const sah_plane* motion_vectors, const sah_plane* history,
                               const sah_plane* out, const sah_taa_upscale_params* params, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_taa_upscale_params) == 28, "sah_taa_upscale_params is 28 bytes");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: params is null");
    if (params->flags & ~(SAH_TAA_HISTORY_INVALID | SAH_TAA_HDR_WEIGHTS)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: unknown flag bits");
    const bool use_history = !(params->flags & SAH_TAA_HISTORY_INVALID);
    const struct {
        const sah_plane* p;
        uint32_t format, bpp;
        const char* what;
    } planes[5] = {{lit, SAH_FORMAT_R16G16B16A16_SFLOAT, 8, "lit must be an R16G16B16A16_SFLOAT plane"},
                   {depth, SAH_FORMAT_D32_SFLOAT, 4, "depth must be a D32_SFLOAT plane"},
                   {motion_vectors, SAH_FORMAT_R16G16_SFLOAT, 4, "motion_vectors must be an R16G16_SFLOAT plane"},
                   {out, SAH_FORMAT_R16G16B16A16_SFLOAT, 8, "out must be an R16G16B16A16_SFLOAT plane"},
                   {history, SAH_FORMAT_R16G16B16A16_SFLOAT, 8, "history must be an R16G16B16A16_SFLOAT plane (NULL only with SAH_TAA_HISTORY_INVALID)"}};
    const int num_planes = use_history ? 5 : 4;  // (a history that is not read is not looked at)
    for (int i = 0; i < num_planes; i++)
        if (const int rc = plane_status(planes[i].p, planes[i].format, planes[i].bpp); rc != SAH_OK)
            return fail(ctx, rc, "taa_upscale: %s, 4-byte aligned, with a pitch of at least a row", planes[i].what);
    const uint32_t w = lit->width, h = lit->height, W = out->width, H = out->height;
    for (int i = 1; i < 3; i++)
        if (planes[i].p->width != w || planes[i].p->height != h)
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: lit, depth and motion_vectors must have one extent (the render resolution)");
    if (use_history && (history->width != W || history->height != H))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: history and out must have one extent (the output resolution)");
    if (w > W || h > H) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: %u x %u to %u x %u is downscaling", w, h, W, H);
    if (too_large(w, h) || too_large(W, H)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: 2^32 texels or more");
    if (row_begin == 0 && row_end == 0) row_end = H;
    if (row_end > H || row_begin > row_end) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bad row range");
    if (!(params->blend > 0.0f && params->blend <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: blend must be in (0, 1]");
    if (!(params->min_confidence >= 0.0f && params->min_confidence <= 1.0f))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: min_confidence must be in [0, 1]");
    for (const float j : {params->jitter[0], params->jitter[1], params->previous_jitter[0], params->previous_jitter[1]})
        if (!std::isfinite(j)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "taa_upscale: a jitter is not finite");
    for (int i = 0; i < num_planes; i++)
        if (i != 3 && overlap(out, 8, planes[i].p, planes[i].bpp))
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
