// C ABI: contrast-adaptive sharpening (include/sah_sharpen.h; kernel in sharpen.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_sharpen.h"
#include "ctx.hpp"
#include "launch.hpp"

extern "C" int sah_sharpen(sah_ctx* ctx, const sah_plane* scene, const sah_exposure_state* exposure, const sah_plane* out, const sah_sharpen_params* params,
                           uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_sharpen_params) == 12, "sah_sharpen_params is 12 bytes");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: params is null");
    if (params->flags & ~SAH_SHARPEN_DENOISE) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: unknown flag bits");
    const PlaneSpec planes[2] = {{scene, SAH_FORMAT_R16G16B16A16_SFLOAT, "scene (R16G16B16A16_SFLOAT)"}, {out, SAH_FORMAT_R16G16B16A16_SFLOAT, "out (R16G16B16A16_SFLOAT)"}};
    if (const int rc = check_planes(ctx, "sharpen", planes, 2); rc != SAH_OK) return rc;
    const uint32_t w = scene->width, h = scene->height;
    if (out->width != w || out->height != h) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: the planes must have one extent");
    if (texel_count_too_large(w, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: 2^32 texels or more");
    if (!resolve_rows(&row_begin, &row_end, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: bad row range");
    if (!(params->sharpness >= 0.0f && params->sharpness <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: sharpness must be in [0, 1]");
    if (!(std::isfinite(params->pre_scale) && params->pre_scale > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: pre_scale must be finite and positive");
    if ((uintptr_t)exposure % 4) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: exposure must be 4-byte aligned");
    const ByteRange target = byte_range(out);
    if (overlaps(target, byte_range(scene))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sharpen: out overlaps scene (the pass reads neighbours: not in place)");
    if (exposure && overlaps(target, byte_range(exposure, sizeof(sah_exposure_state))))
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
