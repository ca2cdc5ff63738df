// C ABI: screen-space ambient occlusion (include/sah_ssao.h; kernels in ssao.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/sah_ssao.h"
#include "ctx.hpp"
#include "launch.hpp"

extern "C" int sah_ssao(sah_ctx* ctx, const sah_view_data* view, const sah_plane* depth, const sah_plane* normals, const sah_plane* scratch,
                        const sah_plane* ao_out, const sah_ssao_params* params, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_ssao_params) == 40, "sah_ssao_params is 40 bytes");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!view || !params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: view or params is null");
    const sah_ssao_params& s = *params;
    if (s.flags) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: no flag is defined");
    if (s.blur_passes > 2) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: blur_passes must be 0, 1 or 2");
    const bool blur = s.blur_passes > 0;
    const PlaneSpec planes[4] = {{depth, SAH_FORMAT_D32_SFLOAT, "depth (D32_SFLOAT)"},
                                 {normals, SAH_FORMAT_R16G16B16A16_SFLOAT, "normals (R16G16B16A16_SFLOAT)"},
                                 {ao_out, SAH_FORMAT_R32_SFLOAT, "ao_out (R32_SFLOAT)"},
                                 {scratch, SAH_FORMAT_R32_SFLOAT, "scratch (R32_SFLOAT; NULL only with blur_passes == 0)"}};
    const int num_planes = blur ? 4 : 3;  // (a scratch that is not used is not looked at)
    if (const int rc = check_planes(ctx, "ssao", planes, num_planes); rc != SAH_OK) return rc;
    const uint32_t w = ao_out->width, h = ao_out->height;
    for (int i = 0; i < num_planes; i++)
        if (planes[i].p->width != w || planes[i].p->height != h) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: the planes must have one extent");
    if (texel_count_too_large(w, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: 2^32 texels or more");
    if (!resolve_rows(&row_begin, &row_end, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: bad row range");
    for (const float v : {s.radius, s.max_radius_pixels, s.shadow_multiplier, s.shadow_clamp, s.horizon_angle_threshold, s.fade_out_from, s.fade_out_to, s.edge_sharpness})
        if (std::isnan(v)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: a parameter is NaN");
    if (!(std::isfinite(s.radius) && s.radius > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: radius must be finite and positive");
    if (!(s.max_radius_pixels >= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: max_radius_pixels must be at least 1");
    if (!(s.shadow_clamp >= 0.0f && s.shadow_clamp <= 1.0f) || !(s.horizon_angle_threshold >= 0.0f && s.horizon_angle_threshold <= 1.0f))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: shadow_clamp and horizon_angle_threshold must be in [0, 1]");
    if (!(s.fade_out_from < s.fade_out_to)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: fade_out_from must be below fade_out_to");
    const float* P = view->projection;
    const float* V = view->view;
    for (const float v : {P[0], P[5], P[8], P[9], view->z_near, V[0], V[1], V[2], V[4], V[5], V[6], V[8], V[9], V[10]})
        if (std::isnan(v)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: a field of the view that the pass reads is NaN");
    if (!(std::isfinite(view->z_near) && view->z_near > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: z_near must be finite and positive");
    for (int i = 0; i < 2; i++) {
        if (overlaps(byte_range(ao_out), byte_range(planes[i].p))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: ao_out overlaps an input (the taps read any row of depth)");
        if (blur && overlaps(byte_range(scratch), byte_range(planes[i].p))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: scratch overlaps an input");
    }
    if (blur && overlaps(byte_range(scratch), byte_range(ao_out))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: scratch overlaps ao_out");
    sah::SsaoArgs a{};
    a.depth = parg(depth), a.normals = parg(normals), a.out = parg(ao_out);
    a.raw = blur ? parg(scratch) : a.out;
    a.W = w, a.H = h, a.row_begin = row_begin, a.row_end = row_end;
    a.raw_begin = row_begin - std::min(row_begin, s.blur_passes);
    a.raw_end = std::min(h, row_end + s.blur_passes);
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) a.m[3 * c + r] = V[4 * c + r];
    const float wf = (float)w, hf = (float)h;
    a.p20 = P[8], a.p21 = P[9], a.ipx = 1.0f / P[0], a.ipy = 1.0f / P[5], a.tx = 2.0f / wf, a.ty = 2.0f / hf;
    a.sx = (0.5f * wf) * P[0];
    a.rs = s.radius * a.sx;
    a.z_near = view->z_near;
    a.max_radius_pixels = s.max_radius_pixels, a.threshold = s.horizon_angle_threshold, a.shadow_multiplier = s.shadow_multiplier, a.shadow_clamp = s.shadow_clamp;
    a.fade_to = s.fade_out_to, a.fade_span = s.fade_out_to - s.fade_out_from, a.edge_sharpness = s.edge_sharpness;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_ssao(a, s.blur_passes, ctx->stream));
    return SAH_OK;
}
