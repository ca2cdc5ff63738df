// C ABI: sky LUTs, the AO clear and the irradiance-cache probe maintenance (kernels in sky_luts.hip, post.hip, probes.hip).
#include <hip/hip_runtime.h>

#include "../../include/sah_hip.h"
#include "ctx.hpp"
#include "launch.hpp"

extern "C" {

int sah_sky_update_luts(sah_ctx* ctx, const sah_plane* transmittance, const sah_plane* multiscattering, const sah_plane* sky_view,
                        const float light_vector[3]) {
    SAH_RANGE();
    if (!ctx || !light_vector) return SAH_ERR_INVALID_ARGUMENT;
    auto ok = [](const sah_plane* p, uint32_t w, uint32_t h) { return rgba16f_ok(p) && p->width == w && p->height == h; };
    if (!ok(transmittance, 256, 64) || !ok(multiscattering, 32, 32) || !ok(sky_view, 200, 200))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "sky LUTs must be RGBA16F 256x64 (transmittance), 32x32 (multiple scattering), 200x200 (sky view)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_sky_luts(parg(transmittance), parg(multiscattering), parg(sky_view), light_vector, ctx->stream));
    return SAH_OK;
}

int sah_ao_clear(sah_ctx* ctx, const sah_plane* ao) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!ao || !ao->ptr || ao->format != SAH_FORMAT_R32_SFLOAT || !ao->width || !ao->height || (uint64_t)ao->row_pitch_bytes < (uint64_t)ao->width * 4 ||
        ((uintptr_t)ao->ptr % 4) || (ao->row_pitch_bytes % 4))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "the AO target must be an R32_SFLOAT plane");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_fill_r32f(parg(ao), ao->width, ao->height, 1.0f, ctx->stream));
    return SAH_OK;
}

// ---- irradiance-cache probe maintenance (a11) ---------------------------------------------------------------------------
static bool probe_vol_ok(const sah_volume& v, uint32_t format, uint32_t bpp, uint32_t w, uint32_t h) {
    return v.ptr && v.format == format && v.width == w && v.height == h && v.depth == 32 && (uint64_t)v.row_pitch_bytes >= (uint64_t)w * bpp &&
           (uint64_t)v.slice_pitch_bytes >= (uint64_t)v.row_pitch_bytes * h && ((uintptr_t)v.ptr % 4) == 0 && (bpp == 1 || (v.row_pitch_bytes % 4) == 0) &&
           (bpp == 1 || (v.slice_pitch_bytes % 4) == 0);
}
static int probe_atlases_args(sah_ctx* ctx, const sah_probe_atlases* a, sah::ProbeAtlasArgs* out) {
    if (!a) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "null probe atlases");
    // extents of irradiance_cache.cpp:94-183: probe grid 32 x (8 * 4) x 32, blocks 7x8 / 13x13 / 12x12 / 1x1
    if (!probe_vol_ok(a->rtgi, SAH_FORMAT_B10G11R11_UFLOAT_PACK32, 4, 32 * 7, 32 * 8) ||
        !probe_vol_ok(a->light_cache, SAH_FORMAT_B10G11R11_UFLOAT_PACK32, 4, 32 * 13, 32 * 13) ||
        !probe_vol_ok(a->depth, SAH_FORMAT_R16G16_SFLOAT, 4, 32 * 12, 32 * 12) || !probe_vol_ok(a->average, SAH_FORMAT_B10G11R11_UFLOAT_PACK32, 4, 32, 32) ||
        !probe_vol_ok(a->validity, SAH_FORMAT_R8_UNORM, 1, 32, 32))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT,
                    "probe atlases must be rtgi 224x256x32 B10G11R11, light cache 416x416x32 B10G11R11, depth 384x384x32 R16G16F, "
                    "average 32x32x32 B10G11R11, validity 32x32x32 R8_UNORM");
    out->rtgi = varg(a->rtgi);
    out->light_cache = varg(a->light_cache);
    out->depth = varg(a->depth);
    out->average = varg(a->average);
    out->validity = varg(a->validity);
    return SAH_OK;
}

int sah_probe_copy(sah_ctx* ctx, const sah_probe_atlases* src, const sah_probe_atlases* dst, const float cascade_movement[4][3]) {
    SAH_RANGE();
    if (!ctx || !cascade_movement) return SAH_ERR_INVALID_ARGUMENT;
    sah::ProbeAtlasArgs s, d;
    int rc = probe_atlases_args(ctx, src, &s);
    if (rc != SAH_OK) return rc;
    rc = probe_atlases_args(ctx, dst, &d);
    if (rc != SAH_OK) return rc;
    if (s.rtgi.ptr == d.rtgi.ptr || s.light_cache.ptr == d.light_cache.ptr || s.depth.ptr == d.depth.ptr || s.average.ptr == d.average.ptr ||
        s.validity.ptr == d.validity.ptr)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "probe copy: source and destination atlases must not alias");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->irr32_copy.drop(ctx->cache_epoch);  // the Lighting pass's fp32 copy of an irradiance atlas is stale from here on
    HIP_TRY(ctx, sah::launch_probe_copy(s, d, cascade_movement, ctx->stream));
    return SAH_OK;
}

int sah_probe_update(sah_ctx* ctx, const sah_probe_atlases* atlases, const sah_volume* trace_results, const uint32_t* probes_to_update,
                     uint32_t num_probes) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    sah::ProbeAtlasArgs a;
    const int rc = probe_atlases_args(ctx, atlases, &a);
    if (rc != SAH_OK) return rc;
    if (num_probes == 0) return SAH_OK;
    if (!probes_to_update) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "probes_to_update is null");
    if (!trace_results || !trace_results->ptr || trace_results->format != SAH_FORMAT_R16G16B16A16_SFLOAT || trace_results->width != 20 ||
        trace_results->height != 20 || trace_results->depth < num_probes || trace_results->row_pitch_bytes < 20 * 8 ||
        (uint64_t)trace_results->slice_pitch_bytes < (uint64_t)trace_results->row_pitch_bytes * 20 || ((uintptr_t)trace_results->ptr % 8) ||
        (trace_results->row_pitch_bytes % 8) || (trace_results->slice_pitch_bytes % 8))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "trace_results must be R16G16B16A16_SFLOAT 20 x 20 x >= num_probes, 8-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the Lighting pass's fp32 copy of this irradiance atlas: kept current probe by probe when the context tracks it
    // (SAH_GENERATION_TRACKED, made from this very atlas), stale otherwise
    const bool patch_irr32 = ctx->irr32_copy.patchable_for(a.rtgi);
    if (!patch_irr32) ctx->irr32_copy.drop(ctx->cache_epoch);
    if (!ctx->probe_slots) {  // probe cell -> position in the update list (probes.hip: ordered_stores); all zero between calls
        HIP_TRY(ctx, hipMalloc((void**)&ctx->probe_slots, 32 * 32 * 32 * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->probe_slots, 0, 32 * 32 * 32 * sizeof(uint32_t), ctx->stream));
    }
    // the slot table is context-wide: an update enqueued on another stream than the previous one starts behind that one's clear pass
    if (!ctx->probe_done) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->probe_done, hipEventDisableTiming));
    if (ctx->probe_stream && ctx->probe_stream != ctx->stream) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->probe_done, 0));
    HIP_TRY(ctx, sah::launch_probe_update(a, varg(*trace_results), probes_to_update, num_probes, ctx->probe_slots, ctx->stream));
    if (patch_irr32) {
        HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_lighting));
        HIP_TRY(ctx, sah::launch_probe_irr_unpack_probes(a.rtgi, ctx->irr32_copy.data(), probes_to_update, num_probes, ctx->stream));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->probe_done, ctx->stream));
    ctx->probe_stream = ctx->stream;
    return SAH_OK;
}

int sah_probe_notify_updated(sah_ctx* ctx, const sah_volume* probe_irradiance, const uint32_t* probes, uint32_t num_probes) {
    SAH_RANGE();
    if (!ctx || !probe_irradiance) return SAH_ERR_INVALID_ARGUMENT;
    if (num_probes == 0) return SAH_OK;
    if (!probes) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "probes is null");
    const sah::VolumeArg irr = varg(*probe_irradiance);
    if (!ctx->irr32_copy.patchable_for(irr)) return SAH_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_lighting));
    HIP_TRY(ctx, sah::launch_probe_irr_unpack_probes(irr, ctx->irr32_copy.data(), probes, num_probes, ctx->stream));
    return SAH_OK;
}

}  // extern "C"
