// C ABI: temporal accumulation and variance-guided filter for the RTGI ray planes (include/sah_rtgi_denoise.h; kernels in rtgi_denoise.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/sah_rtgi_denoise.h"
#include "ctx.hpp"
#include "launch.hpp"

namespace {
struct Checked {
    PlaneSpec spec;
    bool output, previous;  // previous: one of the three planes SAH_RTGI_DENOISE_HISTORY_INVALID excuses
};
}  // namespace

extern "C" int sah_rtgi_denoise(sah_ctx* ctx, const sah_view_data* view, const sah_rtgi_denoise_desc* desc, const sah_rtgi_denoise_params* params,
                                uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_rtgi_denoise_params) == 52, "sah_rtgi_denoise_params is 52 bytes");
    static_assert(sizeof(sah_rtgi_denoise_desc) == 12 * sizeof(void*), "sah_rtgi_denoise_desc is twelve pointers");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!view || !desc || !params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: view, desc or params is null");
    const sah_rtgi_denoise_params& s = *params;
    if (s.flags & ~SAH_RTGI_DENOISE_HISTORY_INVALID) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: unknown flag bits");
    const bool history = !(s.flags & SAH_RTGI_DENOISE_HISTORY_INVALID);
    if (s.passes > 3 || s.normal_squarings > 7) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: passes must be 0..3 and normal_squarings 0..7");
    constexpr uint32_t RGBA16 = SAH_FORMAT_R16G16B16A16_SFLOAT, RGBA32 = SAH_FORMAT_R32G32B32A32_SFLOAT, RG32 = SAH_FORMAT_R32G32_SFLOAT;
    constexpr int kPlanes = 12;
    const Checked planes[kPlanes] = {{{desc->ray_buffer, RGBA16, "ray_buffer (R16G16B16A16_SFLOAT)"}, false, false},
                                     {{desc->ray_irradiance, RGBA16, "ray_irradiance (R16G16B16A16_SFLOAT)"}, false, false},
                                     {{desc->depth, SAH_FORMAT_D32_SFLOAT, "depth (D32_SFLOAT)"}, false, false},
                                     {{desc->normals, RGBA16, "normals (R16G16B16A16_SFLOAT)"}, false, false},
                                     {{desc->motion_vectors, SAH_FORMAT_R16G16_SFLOAT, "motion_vectors (R16G16_SFLOAT)"}, false, false},
                                     {{desc->previous_depth, SAH_FORMAT_D32_SFLOAT, "previous_depth (D32_SFLOAT)"}, false, true},
                                     {{desc->history, RGBA32, "history (R32G32B32A32_SFLOAT)"}, false, true},
                                     {{desc->history_moments, RG32, "history_moments (R32G32_SFLOAT)"}, false, true},
                                     {{desc->accum_out, RGBA32, "accum_out (R32G32B32A32_SFLOAT)"}, true, false},
                                     {{desc->moments_out, RG32, "moments_out (R32G32_SFLOAT)"}, true, false},
                                     {{desc->denoised_ray_buffer, RGBA16, "denoised_ray_buffer (R16G16B16A16_SFLOAT)"}, true, false},
                                     {{desc->denoised_irradiance, RGBA16, "denoised_irradiance (R16G16B16A16_SFLOAT)"}, true, false}};
    const auto used = [history](const Checked& c) { return history || !c.previous; };  // (a previous-frame plane that is not used is not looked at)
    for (const Checked& c : planes)
        if (used(c))
            if (const int rc = check_planes(ctx, "rtgi_denoise", &c.spec, 1); rc != SAH_OK) return rc;
    const uint32_t w = desc->denoised_irradiance->width, h = desc->denoised_irradiance->height;
    for (const Checked& c : planes)
        if (used(c) && (c.spec.p->width != w || c.spec.p->height != h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: the planes must have one extent");
    if (texel_count_too_large(w, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: 2^32 texels or more");
    if (!resolve_rows(&row_begin, &row_end, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: bad row range");
    if (!(s.max_history >= 1.0f && s.max_history <= 256.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: max_history must be in [1, 256]");
    if (!(s.min_history >= 1.0f && s.min_history <= 256.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: min_history must be in [1, 256]");
    if (!(std::isfinite(s.depth_tolerance) && s.depth_tolerance > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: depth_tolerance must be finite and positive");
    if (!(std::isfinite(s.depth_sharpness) && s.depth_sharpness >= 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: depth_sharpness must be finite and not negative");
    if (!(std::isfinite(s.luminance_sigma) && s.luminance_sigma >= 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: luminance_sigma must be finite and not negative");
    if (!(std::isfinite(s.luminance_floor) && s.luminance_floor > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: luminance_floor must be finite and positive");
    for (const float v : {s.jitter[0], s.jitter[1], s.previous_jitter[0], s.previous_jitter[1]})
        if (!std::isfinite(v)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: a jitter is not finite");
    const float* P = view->projection;
    const float* IV = view->inverse_view;
    const float* L = view->last_frame_view;
    for (const float v : {P[0], P[5], P[8], P[9], view->z_near, IV[0], IV[1], IV[2], IV[4], IV[5], IV[6], IV[8], IV[9], IV[10], IV[12], IV[13], IV[14], L[2], L[6], L[10], L[14]})
        if (std::isnan(v)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: a field of the view that the pass reads is NaN");
    if (!(std::isfinite(view->z_near) && view->z_near > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: z_near must be finite and positive");
    for (int o = 0; o < kPlanes; o++)
        for (int i = 0; planes[o].output && i < kPlanes; i++)
            if (i != o && used(planes[i]) && overlaps(byte_range(planes[o].spec.p), byte_range(planes[i].spec.p))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rtgi_denoise: an output overlaps an input or another output");
    sah::RtgiDenoiseArgs a{};
    a.rays = parg(desc->ray_buffer), a.irr = parg(desc->ray_irradiance), a.depth = parg(desc->depth), a.normals = parg(desc->normals), a.mv = parg(desc->motion_vectors);
    if (history) a.prev_depth = parg(desc->previous_depth), a.history = parg(desc->history), a.hist_mom = parg(desc->history_moments);
    a.accum = parg(desc->accum_out), a.moments = parg(desc->moments_out), a.out_rays = parg(desc->denoised_ray_buffer), a.out_irr = parg(desc->denoised_irradiance);
    a.W = w, a.H = h, a.row_begin = row_begin, a.row_end = row_end;
    const uint32_t reach = (1u << s.passes) - 1;
    a.acc_begin = row_begin - std::min(row_begin, reach);
    a.acc_end = std::min(h, row_end + reach);
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 3; r++) a.iv[3 * c + r] = IV[4 * c + r];
    for (int c = 0; c < 4; c++) a.l2[c] = L[4 * c + 2];
    const float wf = (float)w, hf = (float)h;
    a.p20 = P[8], a.p21 = P[9], a.ipx = 1.0f / P[0], a.ipy = 1.0f / P[5], a.tx = 2.0f / wf, a.ty = 2.0f / hf;
    a.z_near = view->z_near;
    a.djx = s.previous_jitter[0] - s.jitter[0], a.djy = s.previous_jitter[1] - s.jitter[1];
    a.max_history = s.max_history, a.min_history = s.min_history, a.depth_tolerance = s.depth_tolerance, a.depth_sharpness = s.depth_sharpness;
    a.luminance_sigma = s.luminance_sigma, a.luminance_floor = s.luminance_floor, a.normal_squarings = s.normal_squarings;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_rtgi_denoise(a, s.passes, history, ctx->stream));
    return SAH_OK;
}
