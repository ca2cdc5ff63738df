// C ABI: screen-space ambient occlusion (include/sah_ssao.h; kernels in ssao.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/sah_ssao.h"
#include "ctx.hpp"
#include "launch.hpp"

namespace {
// 0, or the status a plane of `format` with `bpp`-byte texels earns (the alignment rules of sah_taa_resolve)
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
}  // namespace

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
    const struct {
        const sah_plane* p;
        uint32_t format, bpp;
        const char* what;
    } planes[4] = {{depth, SAH_FORMAT_D32_SFLOAT, 4, "depth must be a D32_SFLOAT plane"},
                   {normals, SAH_FORMAT_R16G16B16A16_SFLOAT, 8, "normals must be an R16G16B16A16_SFLOAT plane"},
                   {ao_out, SAH_FORMAT_R32_SFLOAT, 4, "ao_out must be an R32_SFLOAT plane"},
                   {scratch, SAH_FORMAT_R32_SFLOAT, 4, "scratch must be an R32_SFLOAT plane (NULL only with blur_passes == 0)"}};
    const int num_planes = blur ? 4 : 3;  // (a scratch that is not used is not looked at)
    for (int i = 0; i < num_planes; i++)
        if (const int rc = plane_status(planes[i].p, planes[i].format, planes[i].bpp); rc != SAH_OK)
            return fail(ctx, rc, "ssao: %s, 4-byte aligned, with a pitch of at least a row", planes[i].what);
    const uint32_t w = ao_out->width, h = ao_out->height;
    for (int i = 0; i < num_planes; i++)
        if (planes[i].p->width != w || planes[i].p->height != h) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: the planes must have one extent");
    if (((w | h) >> 31) || (uint64_t)w * h >= (1ull << 32)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: 2^32 texels or more");
    if (row_begin == 0 && row_end == 0) row_end = h;
    if (row_end > h || row_begin > row_end) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: bad row range");
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
        if (overlap(ao_out, 4, planes[i].p, planes[i].bpp)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: ao_out overlaps an input (the taps read any row of depth)");
        if (blur && overlap(scratch, 4, planes[i].p, planes[i].bpp)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: scratch overlaps an input");
    }
    if (blur && overlap(scratch, 4, ao_out, 4)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssao: scratch overlaps ao_out");
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
