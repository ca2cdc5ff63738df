// C ABI: LPV maintenance — sah_lpv_clear, sah_lpv_propagate(_gv) and the two geometry-volume injections (kernels in lpv.hip, lpv_gv.hip).
#include <hip/hip_runtime.h>

#include "../../include/sah_hip.h"
#include "../../include/sah_lpv_gv.h"
#include "ctx.hpp"
#include "launch.hpp"

namespace {
bool lpv_vol_ok(const sah_volume* v) {
    return v && v->ptr && v->format == SAH_FORMAT_R16G16B16A16_SFLOAT && (uint64_t)v->row_pitch_bytes >= (uint64_t)v->width * 8 &&
           (uint64_t)v->slice_pitch_bytes >= (uint64_t)v->row_pitch_bytes * v->height && ((uintptr_t)v->ptr % 8) == 0 &&
           (v->row_pitch_bytes % 8) == 0 && (v->slice_pitch_bytes % 8) == 0;
}
bool gv_volume_ok(const sah_volume* v, uint32_t num_cascades) {
    return lpv_vol_ok(v) && v->width >= 32 * num_cascades && v->height >= 32 && v->depth >= 32 && (uint64_t)v->width * v->height * v->depth <= (1ull << 26) &&
           (uint64_t)v->slice_pitch_bytes * v->depth < (1ull << 32);
}
// sah_lpv_propagate, with use_gv = 1 when `geometry` is not null (sah_lpv_propagate_gv)
int lpv_propagate(sah_ctx* ctx, const sah_volume a_rgb[3], const sah_volume b_rgb[3], const sah_volume* geometry, uint32_t num_cascades, uint32_t steps) {
    if (!ctx || !a_rgb || !b_rgb || num_cascades == 0 || num_cascades > 4) return SAH_ERR_INVALID_ARGUMENT;
    if (geometry && (!lpv_vol_ok(geometry) || !geometry->width || !geometry->height || !geometry->depth ||
                     (uint64_t)geometry->slice_pitch_bytes * geometry->depth >= (1ull << 32)))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "the geometry volume must be an RGBA16F volume under 4 GiB, 8-byte aligned");
    sah::VolumeArg a[3], b[3];
    for (int i = 0; i < 3; i++) {
        if (!lpv_vol_ok(&a_rgb[i]) || !lpv_vol_ok(&b_rgb[i])) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "LPV volumes must be RGBA16F");
        if (a_rgb[i].width < 32 * num_cascades || a_rgb[i].height < 32 || a_rgb[i].depth < 32 || b_rgb[i].width < 32 * num_cascades ||
            b_rgb[i].height < 32 || b_rgb[i].depth < 32)
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "LPV volumes must be at least (32*cascades)x32x32");
        a[i] = varg(a_rgb[i]);
        b[i] = varg(b_rgb[i]);
    }
    // (arguments are in order: from here on the volumes change, and the Lighting pass's gather copy of them is stale — SahLpvCopy::begin_rewrite;
    // only the success path, at the end, says what the copy is now)
    SahLpvCopy& copy = ctx->lpv_copy;
    const SahLpvCopy::Rewrite was = copy.begin_rewrite(ctx->cache_epoch);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->lpv_tables_built) {  // the 30 direction pairs' SH / lobe vectors, into this device's constant memory, once per context
        HIP_TRY(ctx, sah::launch_lpv_build_tables(ctx->stream, &ctx->lpv_hot_structure));
        ctx->lpv_tables_built = true;
    }
    // lpv.hip: the hot form of the 30 direction pairs (finite coefficients) when the tables the device built have the structure it relies on;
    // the general form for a context under sah_debug_set(force_general) — the tests' cross-check
    bool offsets32 = true;  // (the hot kernels address a volume by 32-bit byte offsets)
    for (int i = 0; i < 3; i++)
        offsets32 = offsets32 && (uint64_t)a[i].slice_pitch * a[i].depth < (1ull << 32) && (uint64_t)b[i].slice_pitch * b[i].depth < (1ull << 32);
    const bool hot = ctx->lpv_hot_structure && !ctx->force_general && offsets32;
    // light_propagation_volume.cpp:1016-1034: `steps` dispatches ping-ponging A -> B -> A ...  (Two steps per launch — 8^3 bricks with
    // their halo in LDS, bit-identical — were measured: 28 us per pair against 2 x 9.3 us, 1.5x the arithmetic in longer dependency
    // chains; not kept.)
    // The LAST step also writes the Lighting pass's gather copy of the volumes it stores (sah_gi::lpv_generation, SAH_GENERATION_TRACKED) when
    // the propagated cells are the whole volume — (32 * cascades) x 32 x 32, the reference's extent: a larger volume has texels no step
    // writes.  The copy's buffer belongs to the state sah_lighting builds and reads, possibly on another stream: same guard.
    sah::LpvPackEmit emit = {};
    bool emits = steps > 0;
    const sah::VolumeArg* last = (steps & 1) ? b : a;  // where the last step stores
    for (int i = 0; i < 3; i++) emits = emits && last[i].width == 32 * num_cascades && last[i].height == 32 && last[i].depth == 32;
    if (emits) {
        const SahLpvPackLayout pk = SahLpvCopy::layout(last[0].width, last[0].height, last[0].depth);
        HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_lighting));
        HIP_TRY(ctx, copy.reserve(ctx->stream, ctx->cache_epoch, pk.total));
        if (!ctx->state) emits = false;  // (made by sah_create; a context without it has no fast Lighting path either)
        if (emits) HIP_TRY(ctx, copy.borders_for(ctx->stream, last[0].width, last[0].height, last[0].depth, pk.total));
        emit = {copy.data(), pk.row_pitch, pk.slice_pitch, ctx->state};
    }
    // use_gv = 1: the GV does not change during the steps, so its 30 factors per cell are computed once, ahead of them, and every step
    // reads them (64 bytes per cell; sampling the GV in every step instead was measured and lost: DESIGN.md §5i, §7)
    sah::LpvGvStep gv = {};
    if (geometry && steps > 0) {
        gv.gv = varg(*geometry);
        HIP_TRY(ctx, ctx->gv_factors.grow(ctx->stream, (size_t)4 * 16 * 32768 * 4));
        gv.factors = ctx->gv_factors.ptr;
        HIP_TRY(ctx, sah::launch_lpv_gv_factors(gv.gv, gv.factors, num_cascades, ctx->stream));
    }
    const sah::LpvGvStep* g = geometry ? &gv : nullptr;
    for (uint32_t s = 0; s < steps; s++) {
        const sah::LpvPackEmit* e = (emits && s + 1 == steps) ? &emit : nullptr;
        if ((s & 1) == 0) HIP_TRY(ctx, sah::launch_lpv_propagate(a, b, num_cascades, e, hot, ctx->stream, g));
        else HIP_TRY(ctx, sah::launch_lpv_propagate(b, a, num_cascades, e, hot, ctx->stream, g));
    }
    copy.commit_rewrite(ctx->cache_epoch, was, emits ? last : nullptr);
    return SAH_OK;
}
}  // namespace

extern "C" {

int sah_lpv_clear(sah_ctx* ctx, const sah_volume* red, const sah_volume* green, const sah_volume* blue, const sah_volume* geometry,
                  uint32_t num_cascades) {
    SAH_RANGE();
    if (ctx) ctx->lpv_copy.drop(ctx->cache_epoch);
    if (!ctx || num_cascades == 0 || num_cascades > 4) return SAH_ERR_INVALID_ARGUMENT;
    const sah_volume* in[4] = {red, green, blue, geometry};
    sah::VolumeArg v[4];
    int n = 0;
    for (const sah_volume* p : in) {
        if (!p || !p->ptr) continue;
        if (!lpv_vol_ok(p)) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "LPV volumes must be RGBA16F, 8-byte aligned");
        v[n++] = varg(*p);
    }
    if (n == 0) return SAH_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_lpv_clear(v, n, num_cascades, ctx->stream));
    return SAH_OK;
}

int sah_lpv_propagate(sah_ctx* ctx, const sah_volume a_rgb[3], const sah_volume b_rgb[3], uint32_t num_cascades, uint32_t steps) {
    SAH_RANGE();
    return lpv_propagate(ctx, a_rgb, b_rgb, nullptr, num_cascades, steps);
}

int sah_lpv_propagate_gv(sah_ctx* ctx, const sah_volume a_rgb[3], const sah_volume b_rgb[3], const sah_volume* geometry, uint32_t num_cascades,
                         uint32_t steps) {
    SAH_RANGE();
    return lpv_propagate(ctx, a_rgb, b_rgb, geometry, num_cascades, steps);
}

// The two GV injections (lpv_gv.hip).  Neither reads or writes the colour volumes: the Lighting pass's gather copy and the cache epoch stay.
int sah_lpv_inject_rsm_gv(sah_ctx* ctx, const sah_rsm_targets* rsm, const sah_lpv_cascade_matrices* cascades, uint32_t first_cascade,
                          uint32_t cascade_count, uint32_t num_cascades, const sah_volume* geometry) {
    SAH_RANGE();
    if (!ctx || !rsm || !cascades || !geometry || num_cascades == 0 || num_cascades > 4) return SAH_ERR_INVALID_ARGUMENT;
    if (first_cascade >= num_cascades || cascade_count > num_cascades - first_cascade)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "cascades [first, first + count) must lie in [0, num_cascades)");
    if (!gv_volume_ok(geometry, num_cascades))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "the geometry volume must be RGBA16F, at least (32*cascades)x32x32, 8-byte aligned");
    const sah_volume& n = rsm->normals;
    const sah_volume& d = rsm->depth;
    const uint32_t layers = first_cascade + cascade_count;
    if (!n.ptr || !d.ptr || n.format != SAH_FORMAT_R8G8B8A8_UNORM || d.format != SAH_FORMAT_D16_UNORM || !d.width || !d.height ||
        n.width != d.width || n.height != d.height || n.depth < layers || d.depth < layers || (uint64_t)d.width * d.height >= (1ull << 31) ||
        (uint64_t)n.row_pitch_bytes < (uint64_t)n.width * 4 || (uint64_t)n.slice_pitch_bytes < (uint64_t)n.row_pitch_bytes * n.height ||
        (uint64_t)d.row_pitch_bytes < (uint64_t)d.width * 2 || (uint64_t)d.slice_pitch_bytes < (uint64_t)d.row_pitch_bytes * d.height ||
        ((uintptr_t)n.ptr % 4) != 0 || (n.row_pitch_bytes % 4) != 0 || (n.slice_pitch_bytes % 4) != 0 || ((uintptr_t)d.ptr % 2) != 0 ||
        (d.row_pitch_bytes % 2) != 0 || (d.slice_pitch_bytes % 2) != 0)
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "RSM: normals R8G8B8A8_UNORM and depth D16_UNORM arrays of equal extents with the cascades' layers");
    if (cascade_count == 0) return SAH_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t need = (size_t)16 * geometry->width * geometry->height * geometry->depth;
    HIP_TRY(ctx, ctx->gv_keys.grow(ctx->stream, need));
    HIP_TRY(ctx, sah::launch_gv_inject_rsm(varg(n), varg(d), cascades, first_cascade, cascade_count, num_cascades, varg(*geometry), (uint32_t*)ctx->gv_keys.ptr,
                                           ctx->stream));
    return SAH_OK;
}

int sah_lpv_inject_scene_gv(sah_ctx* ctx, const sah_plane* depth, const sah_plane* normals, const sah_view_data* view,
                            const sah_lpv_cascade_matrices* cascades, uint32_t num_cascades, const sah_volume* geometry) {
    SAH_RANGE();
    if (!ctx || !depth || !normals || !view || !cascades || !geometry || num_cascades == 0 || num_cascades > 4) return SAH_ERR_INVALID_ARGUMENT;
    if (!gv_volume_ok(geometry, num_cascades))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "the geometry volume must be RGBA16F, at least (32*cascades)x32x32, 8-byte aligned");
    if (!depth->ptr || depth->format != SAH_FORMAT_D32_SFLOAT || !depth->width || !depth->height || (uint64_t)depth->row_pitch_bytes < (uint64_t)depth->width * 4 ||
        ((uintptr_t)depth->ptr % 4) != 0 || (depth->row_pitch_bytes % 4) != 0 || !rgba16f_ok(normals) || normals->width != depth->width ||
        normals->height != depth->height || (uint64_t)depth->width * depth->height >= (1ull << 32))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "scene GV: depth D32_SFLOAT and normals R16G16B16A16_SFLOAT planes of equal extents");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t need = (size_t)16 * geometry->width * geometry->height * geometry->depth;
    HIP_TRY(ctx, ctx->gv_keys.grow(ctx->stream, need));
    HIP_TRY(ctx, sah::launch_gv_inject_scene(parg(depth), parg(normals), depth->width, depth->height, *view, cascades, num_cascades, varg(*geometry),
                                             (uint32_t*)ctx->gv_keys.ptr, ctx->stream));
    return SAH_OK;
}

}  // extern "C"
