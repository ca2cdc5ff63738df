// C ABI: screen-space reflections (include/sah_ssr.h; kernels in ssr.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_ssr.h"
#include "ctx.hpp"
#include "launch.hpp"

extern "C" int sah_ssr(sah_ctx* ctx, const sah_view_data* view, const sah_plane* color, const sah_plane* normals, const sah_plane* data,
                       const sah_plane* depth, const sah_plane* source, const sah_plane* lit, const sah_plane* scratch, const sah_plane* out,
                       const sah_ssr_params* params, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_ssr_params) == 36, "sah_ssr_params is 36 bytes");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!view || !params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: view or params is null");
    const sah_ssr_params& s = *params;
    if (s.flags & ~(SAH_SSR_JITTER | SAH_SSR_REFLECTION_ONLY)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: an undefined flag bit is set");
    const PlaneSpec planes[8] = {{out, SAH_FORMAT_R16G16B16A16_SFLOAT, "out (R16G16B16A16_SFLOAT)"},
                                 {color, SAH_FORMAT_R8G8B8A8_SRGB, "color (R8G8B8A8_SRGB)"},
                                 {normals, SAH_FORMAT_R16G16B16A16_SFLOAT, "normals (R16G16B16A16_SFLOAT)"},
                                 {data, SAH_FORMAT_R8G8B8A8_UNORM, "data (R8G8B8A8_UNORM)"},
                                 {depth, SAH_FORMAT_D32_SFLOAT, "depth (D32_SFLOAT)"},
                                 {source, SAH_FORMAT_R16G16B16A16_SFLOAT, "source (R16G16B16A16_SFLOAT)"},
                                 {lit, SAH_FORMAT_R16G16B16A16_SFLOAT, "lit (R16G16B16A16_SFLOAT)"},
                                 {scratch, SAH_FORMAT_R32_SFLOAT, "scratch (R32_SFLOAT)"}};
    if (const int rc = check_planes(ctx, "ssr", planes, 8); rc != SAH_OK) return rc;
    const uint32_t w = out->width, h = out->height;
    for (int i = 0; i < 7; i++)
        if (planes[i].p->width != w || planes[i].p->height != h) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: the planes must have one extent");
    if (texel_count_too_large(w, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: 2^32 texels or more");
    if (scratch->width != (w + 7) / 8 || scratch->height != (h + 7) / 8)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: scratch must be ceil(W / 8) x ceil(H / 8)");
    if (!resolve_rows(&row_begin, &row_end, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: bad row range");
    for (const float v : {s.max_distance, s.thickness, s.stride_pixels, s.max_roughness, s.edge_fade, s.intensity})
        if (std::isnan(v)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: a parameter is NaN");
    if (!(std::isfinite(s.max_distance) && s.max_distance > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: max_distance must be finite and positive");
    if (!(s.thickness >= 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: thickness must not be negative");
    if (!(std::isfinite(s.stride_pixels) && s.stride_pixels >= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: stride_pixels must be finite and at least 1");
    if (s.max_steps < 1 || s.max_steps > 256) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: max_steps must be in 1..256");
    if (s.refine_steps > 8) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: refine_steps must be in 0..8");
    if (!(s.max_roughness > 0.0f && s.max_roughness <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: max_roughness must be in (0, 1]");
    if (!(s.edge_fade > 0.0f && s.edge_fade <= 0.5f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: edge_fade must be in (0, 0.5]");
    if (!(std::isfinite(s.intensity) && s.intensity >= 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: intensity must be finite and not negative");
    const float* P = view->projection;
    const float* V = view->view;
    for (const float v : {P[0], P[5], P[8], P[9], view->z_near, V[0], V[1], V[2], V[4], V[5], V[6], V[8], V[9], V[10]})
        if (std::isnan(v)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: a field of the view that the pass reads is NaN");
    if (!(std::isfinite(view->z_near) && view->z_near > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: z_near must be finite and positive");
    for (int i = 1; i < 8; i++)
        if (overlaps(byte_range(out), byte_range(planes[i].p)))
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: out overlaps an input or scratch (the rays read any texel of source)");
    for (int i = 1; i < 7; i++)
        if (overlaps(byte_range(scratch), byte_range(planes[i].p))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "ssr: scratch overlaps an input");
    sah::SsrArgs a{};
    a.color = parg(color), a.normals = parg(normals), a.data = parg(data), a.depth = parg(depth), a.source = parg(source), a.lit = parg(lit);
    a.out = parg(out);  // (scratch is reserved: checked above, neither read nor written)
    a.W = w, a.H = h, a.row_begin = row_begin, a.row_end = row_end;
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) a.m[3 * c + r] = V[4 * c + r];
    const float wf = (float)w, hf = (float)h;
    a.p00 = P[0], a.p11 = P[5], a.p20 = P[8], a.p21 = P[9], a.ipx = 1.0f / P[0], a.ipy = 1.0f / P[5], a.tx = 2.0f / wf, a.ty = 2.0f / hf;
    a.hw = 0.5f * wf, a.hh = 0.5f * hf;
    a.z_near = view->z_near;
    a.max_distance = s.max_distance, a.thickness = s.thickness, a.stride = s.stride_pixels, a.max_roughness = s.max_roughness;
    a.edge_fade = s.edge_fade, a.intensity = s.intensity;
    a.max_steps = s.max_steps, a.refine_steps = s.refine_steps, a.flags = s.flags;
    a.luts = ctx->luts;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_ssr(a, ctx->stream));
    return SAH_OK;
}
