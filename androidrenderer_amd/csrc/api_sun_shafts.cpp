// C ABI: volumetric sun light (include/sah_sun_shafts.h; kernels in sun_shafts.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/sah_sun_shafts.h"
#include "ctx.hpp"
#include "launch.hpp"
#include "lighting_stages.hpp"

namespace {
// M * v of the header (numerics.hpp's mul44, on the host: the library is compiled without contraction)
void mul44(const float* m, const float v[4], float r[4]) {
    for (int i = 0; i < 4; i++) r[i] = ((m[i] * v[0] + m[4 + i] * v[1]) + m[8 + i] * v[2]) + m[12 + i] * v[3];
}
}  // namespace

extern "C" int sah_sun_shafts(sah_ctx* ctx, const sah_view_data* view, const sah_sun_light_constants* sun, const sah_volume* shadowmap,
                              const sah_plane* depth, const sah_plane* lit, const sah_plane* march, const sah_plane* out,
                              const sah_sun_shafts_params* params, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_sun_shafts_params) == 60, "sah_sun_shafts_params is 60 bytes");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: params is null");
    if (!view || !sun) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: view and sun are required");
    const sah_sun_shafts_params& s = *params;
    if (s.flags & ~(SAH_SUN_SHAFTS_DITHER | SAH_SUN_SHAFTS_TERM_ONLY)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: an undefined flag bit is set");
    const bool term_only = (s.flags & SAH_SUN_SHAFTS_TERM_ONLY) != 0;
    if (term_only) lit = nullptr;  // not read
    const PlaneSpec planes[4] = {{out, SAH_FORMAT_R16G16B16A16_SFLOAT, "out (R16G16B16A16_SFLOAT)"},
                                 {march, SAH_FORMAT_R16G16B16A16_SFLOAT, "march (R16G16B16A16_SFLOAT)"},
                                 {depth, SAH_FORMAT_D32_SFLOAT, "depth (D32_SFLOAT)"},
                                 {lit, SAH_FORMAT_R16G16B16A16_SFLOAT, "lit (R16G16B16A16_SFLOAT; not looked at with SAH_SUN_SHAFTS_TERM_ONLY)"}};
    const int num_planes = term_only ? 3 : 4;
    if (const int rc = check_planes(ctx, "sun_shafts", planes, num_planes); rc != SAH_OK) return rc;
    const uint32_t w = out->width, h = out->height;
    if (depth->width != w || depth->height != h || (lit && (lit->width != w || lit->height != h)))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: depth, lit and out must have one extent (the render resolution)");
    if (texel_count_too_large(w, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: 2^32 texels or more");
    if (s.downscale != 1 && s.downscale != 2) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: downscale must be 1 or 2");
    const uint32_t mw = (w + s.downscale - 1) / s.downscale, mh = (h + s.downscale - 1) / s.downscale;
    if (march->width != mw || march->height != mh)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: march must be ceil(w / s) x ceil(h / s) = %u x %u", mw, mh);
    if (!resolve_rows(&row_begin, &row_end, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: bad row range");
    for (const float v : {s.step_length, s.step_transmittance, s.albedo[0], s.albedo[1], s.albedo[2], s.ambient[0], s.ambient[1], s.ambient[2], s.anisotropy,
                          s.depth_bias, s.depth_sharpness, view->z_near})
        if (std::isnan(v)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: a parameter is NaN");
    if (!(std::isfinite(s.step_length) && s.step_length > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: step_length must be finite and positive");
    if (!(std::isfinite(view->z_near) && view->z_near > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: the view's z_near must be finite and positive");
    if (s.num_steps < 1 || s.num_steps > SAH_SUN_SHAFTS_MAX_STEPS) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: num_steps must be 1..64");
    if (!(s.step_transmittance > 0.0f && s.step_transmittance <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: step_transmittance must be in (0, 1]");
    for (const float v : {s.albedo[0], s.albedo[1], s.albedo[2], s.ambient[0], s.ambient[1], s.ambient[2], s.depth_bias})
        if (!std::isfinite(v)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: albedo, ambient and depth_bias must be finite");
    if (!(s.anisotropy > -1.0f && s.anisotropy < 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: anisotropy must be in (-1, 1)");
    if (!(std::isfinite(s.depth_sharpness) && s.depth_sharpness >= 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: depth_sharpness must be finite and not negative");
    if (s.dither_offset > 15) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: dither_offset must be 0..15");
    for (int i = 1; i < num_planes; i++)
        if (overlaps(byte_range(out), byte_range(planes[i].p))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: out overlaps depth, lit or march");
    for (int i = 2; i < num_planes; i++)
        if (overlaps(byte_range(march), byte_range(planes[i].p))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: march overlaps depth or lit");

    sah::SunShaftsArgs a;
    memset(&a, 0, sizeof(a));
    if (shadowmap && shadowmap->ptr) {
        const sah_volume& m = *shadowmap;
        if (m.format != SAH_FORMAT_D16_UNORM && m.format != SAH_FORMAT_D32_SFLOAT)
            return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "sun_shafts: shadowmap must be D16_UNORM or D32_SFLOAT");
        const uint32_t bpp = m.format == SAH_FORMAT_D16_UNORM ? 2 : 4;
        if (!m.width || !m.height || !m.depth || ((m.width | m.height) >> 31) || (uint64_t)m.row_pitch_bytes < (uint64_t)m.width * bpp ||
            (uint64_t)m.slice_pitch_bytes < (uint64_t)m.row_pitch_bytes * m.height || (uint64_t)m.row_pitch_bytes * m.height >= (1ull << 32) ||
            ((uintptr_t)m.ptr % bpp) || (m.row_pitch_bytes % bpp) || (m.slice_pitch_bytes % bpp))
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "sun_shafts: shadowmap needs a layer, an extent, pitches of at least a row and a layer, its texel's alignment and layers below 4 GiB");
        a.csm.shadowmap = varg(m);
        a.csm.is_d16 = bpp == 2;
        sah::csm_d16_conversion(a.csm);
        a.num_cascades = m.depth < 4 ? m.depth : 4;
    }
    const float A4[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    float A[4];
    mul44(view->inverse_view, A4, A);
    A[3] = 1.0f;
    sah::csm_sun_tables(*sun, a.csm);  // Lighting's splits and biased matrices
    for (int c = 0; c < 4; c++) {
        float ac[4];
        mul44(a.csm.biased[c], A, ac);
        for (int i = 0; i < 3; i++) a.a[c][i] = ac[i] / ac[3];
    }
    a.depth = parg(depth), a.march = parg(march), a.out = parg(out);
    if (lit) a.lit = parg(lit);
    a.w = w, a.h = h, a.mw = mw, a.mh = mh, a.row_begin = row_begin, a.row_end = row_end;
    if (row_end > row_begin) {
        a.march_row_begin = s.downscale == 1 ? row_begin : row_begin / 2;
        a.march_row_end = s.downscale == 1 ? row_end : ((row_end - 1) / 2 + 2 < mh ? (row_end - 1) / 2 + 2 : mh);
    }
    a.downscale = s.downscale, a.num_steps = s.num_steps, a.dither_offset = s.dither_offset, a.flags = s.flags;
    a.wf = (float)w, a.hf = (float)h;
    memcpy(a.inv_proj, view->inverse_projection, 64);
    memcpy(a.inv_view, view->inverse_view, 64);
    const float n[3] = {-sun->direction_and_tan_size[0], -sun->direction_and_tan_size[1], -sun->direction_and_tan_size[2]};
    const float inv = 1.0f / std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const float l[3] = {n[0] * inv, n[1] * inv, n[2] * inv};
    for (int r = 0; r < 3; r++) a.lv[r] = (view->view[r] * l[0] + view->view[4 + r] * l[1]) + view->view[8 + r] * l[2];
    for (int i = 0; i < 3; i++) a.sun_color[i] = sun->color[i], a.albedo[i] = s.albedo[i], a.ambient[i] = s.ambient[i];
    a.step_length = s.step_length, a.z_near = view->z_near, a.depth_bias = s.depth_bias, a.depth_sharpness = s.depth_sharpness;
    a.d_min = view->z_near / (s.step_length * (float)s.num_steps);
    const float g = s.anisotropy;
    a.g1 = 1.0f + g * g, a.g2 = 1.0f - g * g, a.g3 = 2.0f * g;
    float P = 1.0f;
    for (uint32_t k = 0; k < s.num_steps; k++) {
        const float next = P * s.step_transmittance;
        a.D[k] = P - next;
        P = next;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_sun_shafts(a, ctx->stream));
    return SAH_OK;
}
