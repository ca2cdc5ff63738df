// C ABI: variable-rate Lighting and the VRSAA resolve (include/sah_vrs.h; kernels in lighting_vrs.hip and vrs_resolve.hip).  The descriptor of
// sah_lighting_vrs is digested by the stages of sah_lighting itself (lighting_stages.hpp): the kernel receives the argument blocks that
// sah_lighting's kernels would.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_vrs.h"
#include "ctx.hpp"
#include "launch.hpp"
#include "lighting_stages.hpp"

namespace {
// log2 of a texel size that is a power of two in [4, 64]; -1 for another
int texel_shift(uint32_t t) {
    for (int s = 2; s <= 6; s++)
        if (t == (1u << s)) return s;
    return -1;
}
}  // namespace

extern "C" {

int sah_lighting_vrs(sah_ctx* ctx, const sah_lighting_vrs_desc* desc) {
    SAH_RANGE();
    using namespace sah;
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!desc || !desc->lighting || !desc->shading_rate_image) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lighting_vrs: desc, its lighting desc and its shading-rate image are required");
    const sah_lighting_desc* d = desc->lighting;
    LightingCall call;
    LightingArgs a;
    CsmArgs csm;
    LpvArgs lpv;
    SkyArgs sky;
    if (const int rc = lighting_targets(ctx, d, call, a); rc != SAH_OK) return rc;
    if (call.gi_kind == SAH_GI_CACHE || call.gi_kind == SAH_GI_RTGI)
        return fail(ctx, SAH_ERR_UNSUPPORTED, "lighting_vrs: GI kind %u is not shaded at a variable rate (none and LPV are)", call.gi_kind);
    if (d->lights && d->lights->count) return fail(ctx, SAH_ERR_UNSUPPORTED, "lighting_vrs: a light list is not shaded at a variable rate");
    if (const int rc = lighting_csm(ctx, d, call, csm); rc != SAH_OK) return rc;
    if (const int rc = lighting_gi_lpv(ctx, d, call, lpv); rc != SAH_OK) return rc;
    if (const int rc = lighting_sky(ctx, d, sky); rc != SAH_OK) return rc;

    const sah_plane* s = desc->shading_rate_image;
    if (!s->ptr) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lighting_vrs: the shading-rate image has no memory");
    if (s->format != SAH_FORMAT_R8_UINT) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "lighting_vrs: the shading-rate image must be an R8_UINT plane");
    const int sx = texel_shift(desc->texel_size[0]), sy = texel_shift(desc->texel_size[1]);
    if (sx < 0 || sy < 0)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lighting_vrs: texel size %u x %u is not a power of two in [4, 64] per axis", desc->texel_size[0], desc->texel_size[1]);
    const uint32_t need_w = (call.W - 1u) / desc->texel_size[0] + 1u, need_h = (call.H - 1u) / desc->texel_size[1] + 1u;
    if (s->width < need_w || s->height < need_h)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lighting_vrs: a %u x %u shading-rate image does not cover the frame (%u x %u texels)", s->width, s->height, need_w, need_h);
    if (s->row_pitch_bytes < s->width) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lighting_vrs: the shading-rate image's pitch is below its width");
    if (!(desc->depth_tolerance >= 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lighting_vrs: depth_tolerance must not be negative or NaN");
    if (call.r0 % 4u != 0u || (call.r1 % 4u != 0u && call.r1 != call.H))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lighting_vrs: row range [%u,%u): row_begin must be a multiple of 4, row_end a multiple of 4 or the height", call.r0, call.r1);

    VrsArgs v{};
    v.rate = parg(s);
    v.texel_shift[0] = (uint32_t)sx;
    v.texel_shift[1] = (uint32_t)sy;
    v.depth_tolerance = desc->depth_tolerance;
    v.vec4 = call.vec4ok ? 1u : 0u;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_lighting_vrs(a, csm, lpv, sky, v, (int)call.sun_mode, (int)call.gi_kind, ctx->stream));
    return SAH_OK;
}

int sah_vrsaa_resolve(sah_ctx* ctx, const sah_plane* lit, const sah_plane* antialiased, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    const struct {
        const sah_plane* p;
        const char* what;
    } planes[2] = {{lit, "lit"}, {antialiased, "antialiased"}};
    for (const auto& pl : planes) {
        if (!pl.p || !pl.p->ptr) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "vrsaa_resolve: %s is null", pl.what);
        if (pl.p->format != SAH_FORMAT_R16G16B16A16_SFLOAT) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "vrsaa_resolve: %s must be R16G16B16A16_SFLOAT", pl.what);
        if (!rgba16f_ok(pl.p)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "vrsaa_resolve: %s must be 8-byte aligned, not empty, with a pitch of at least a row", pl.what);
    }
    const uint32_t w = antialiased->width, h = antialiased->height;
    if ((uint64_t)lit->width != 2ull * w || (uint64_t)lit->height != 2ull * h)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "vrsaa_resolve: lit is %u x %u, not twice the %u x %u of antialiased", lit->width, lit->height, w, h);
    if (row_begin == 0 && row_end == 0) row_end = h;
    if (row_end > h || row_begin > row_end) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "vrsaa_resolve: bad row range");
    if (overlaps(byte_range(lit), byte_range(antialiased))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "vrsaa_resolve: the planes overlap");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_vrsaa_resolve(parg(lit), parg(antialiased), w, h, row_begin, row_end, ctx->stream));
    return SAH_OK;
}

}  // extern "C"
