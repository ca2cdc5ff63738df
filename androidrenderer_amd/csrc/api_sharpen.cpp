// C ABI: contrast-adaptive sharpening (include/sah_sharpen.h; kernel in sharpen.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_sharpen.h"
#include "ctx.hpp"
#include "launch.hpp"

namespace {
struct Range {
    uintptr_t begin, end;
};
Range range_of(const sah_plane* p) {
    const uintptr_t b = (uintptr_t)p->ptr;
    return {b, b + (uint64_t)(p->height - 1) * p->row_pitch_bytes + (uint64_t)p->width * 8};
}
bool overlap(const Range& a, const Range& b) { return a.begin < b.end && b.begin < a.end; }

// 0, or the status an R16G16B16A16_SFLOAT plane earns (the alignment rules of sah_taa_resolve)
int plane_status(const sah_plane* p) {
    if (!p || !p->ptr) return SAH_ERR_INVALID_ARGUMENT;
    if (p->format != SAH_FORMAT_R16G16B16A16_SFLOAT) return SAH_ERR_UNSUPPORTED_FORMAT;
    if (!p->width || !p->height || (uint64_t)p->row_pitch_bytes < (uint64_t)p->width * 8 || ((uintptr_t)p->ptr % 4) || (p->row_pitch_bytes % 4))
        return SAH_ERR_INVALID_ARGUMENT;
    return SAH_OK;
}
}  // namespace

extern "C" int sah_sharpen(sah_ctx* ctx, const sah_plane* scene, const sah_exposure_state* exposure, const sah_plane* out, const sah_sharpen_params* params,
                           uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_sharpen_params) == 12, "sah_sharpen_params is 12 bytes");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: params is null");
    if (params->flags & ~SAH_SHARPEN_DENOISE) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: unknown flag bits");
    const struct {
        const sah_plane* p;
        const char* what;
    } planes[2] = {{scene, "scene"}, {out, "out"}};
    for (const auto& pl : planes)
        if (const int rc = plane_status(pl.p); rc != SAH_OK)
            return fail(ctx, rc, "sharpen: %s must be an R16G16B16A16_SFLOAT plane, 4-byte aligned, with a pitch of at least a row", pl.what);
    const uint32_t w = scene->width, h = scene->height;
    if (out->width != w || out->height != h) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: the planes must have one extent");
    if (((w | h) >> 31) || (uint64_t)w * h >= (1ull << 32)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: 2^32 texels or more");
    if (row_begin == 0 && row_end == 0) row_end = h;
    if (row_end > h || row_begin > row_end) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: bad row range");
    if (!(params->sharpness >= 0.0f && params->sharpness <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: sharpness must be in [0, 1]");
    if (!(std::isfinite(params->pre_scale) && params->pre_scale > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: pre_scale must be finite and positive");
    if ((uintptr_t)exposure % 4) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: exposure must be 4-byte aligned");
    const Range target = range_of(out);
    if (overlap(target, range_of(scene))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: out overlaps scene (the pass reads neighbours: not in place)");
    if (exposure && overlap(target, Range{(uintptr_t)exposure, (uintptr_t)exposure + sizeof(sah_exposure_state)}))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: out overlaps the exposure state");
    sah::SharpenArgs a{};
    a.scene = parg(scene), a.out = parg(out);
    a.W = w, a.H = h, a.row_begin = row_begin, a.row_end = row_end;
    a.exposure = exposure;
    a.sharpness = params->sharpness, a.pre_scale = params->pre_scale;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_sharpen(a, (params->flags & SAH_SHARPEN_DENOISE) != 0, ctx->stream));
    return SAH_OK;
}
