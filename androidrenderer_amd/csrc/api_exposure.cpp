// C ABI: histogram auto-exposure (include/sah_exposure.h; kernels in exposure.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_exposure.h"
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
Range range_of(const void* p, uint64_t bytes) { return {(uintptr_t)p, (uintptr_t)p + bytes}; }
bool overlap(const Range& a, const Range& b) { return a.begin < b.end && b.begin < a.end; }

// 0, or the status an R16G16B16A16_SFLOAT plane earns (the alignment rules of sah_taa_resolve)
int plane_status(const sah_plane* p) {
    if (!p || !p->ptr) return SAH_ERR_INVALID_ARGUMENT;
    if (p->format != SAH_FORMAT_R16G16B16A16_SFLOAT) return SAH_ERR_UNSUPPORTED_FORMAT;
    if (!p->width || !p->height || (uint64_t)p->row_pitch_bytes < (uint64_t)p->width * 8 || ((uintptr_t)p->ptr % 4) || (p->row_pitch_bytes % 4))
        return SAH_ERR_INVALID_ARGUMENT;
    return SAH_OK;
}
// scene and a target of it: one extent below 2^32 texels; the target is the scene's plane itself or disjoint from it
const char* pair_problem(const sah_plane* scene, const sah_plane* target) {
    if (((scene->width | scene->height) >> 31) || (uint64_t)scene->width * scene->height >= (1ull << 32)) return "2^32 texels or more";
    if (!target) return nullptr;
    if (target->width != scene->width || target->height != scene->height) return "the planes must have one extent";
    const bool same = target->ptr == scene->ptr && target->row_pitch_bytes == scene->row_pitch_bytes;
    if (!same && overlap(range_of(scene), range_of(target))) return "the target overlaps the scene without being the same plane";
    return nullptr;
}
bool positive_finite(float v) { return std::isfinite(v) && v > 0.0f; }
}  // namespace

extern "C" int sah_exposure_meter(sah_ctx* ctx, const sah_plane* scene, const sah_exposure_state* state_in, sah_exposure_state* state_out, void* work,
                                  const sah_plane* exposed_out, const sah_exposure_params* params) {
    SAH_RANGE();
    static_assert(sizeof(sah_exposure_params) == 32, "sah_exposure_params is 32 bytes");
    static_assert(sizeof(sah_exposure_state) == 16, "sah_exposure_state is 16 bytes");
    static_assert(SAH_EXPOSURE_WORK_BYTES == (SAH_EXPOSURE_BINS + 4) * 4, "256 bins, the ticket word, three reserved words");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!params || !state_out || !work) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: params, state_out or work is null");
    const sah_exposure_params& s = *params;
    if (s.flags & ~SAH_EXPOSURE_HISTORY_INVALID) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: unknown flag bits");
    const bool history = !(s.flags & SAH_EXPOSURE_HISTORY_INVALID);
    if (history && !state_in) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: state_in may be null only with SAH_EXPOSURE_HISTORY_INVALID");
    if (!history && exposed_out) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: the fused form needs a history (the first frame calls meter, then apply)");
    if (const int rc = plane_status(scene); rc != SAH_OK)
        return fail(ctx, rc, "exposure_meter: scene must be an R16G16B16A16_SFLOAT plane, 4-byte aligned, with a pitch of at least a row");
    if (exposed_out)
        if (const int rc = plane_status(exposed_out); rc != SAH_OK)
            return fail(ctx, rc, "exposure_meter: exposed_out must be an R16G16B16A16_SFLOAT plane, 4-byte aligned, with a pitch of at least a row");
    if (const char* why = pair_problem(scene, exposed_out)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: %s", why);
    if (!positive_finite(s.key) || !positive_finite(s.min_exposure) || !positive_finite(s.max_exposure) || s.min_exposure > s.max_exposure)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: key, min_exposure and max_exposure must be finite and positive, min <= max");
    if (!(s.low_fraction >= 0.0f && s.low_fraction < s.high_fraction && s.high_fraction <= 1.0f))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: the fractions must be 0 <= low < high <= 1");
    if (!(s.adaptation > 0.0f && s.adaptation <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: adaptation must be in (0, 1]");
    if (((uintptr_t)work % 4) || ((uintptr_t)state_out % 4) || (history && ((uintptr_t)state_in % 4)))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: work and the states must be 4-byte aligned");
    // work, state_out, state_in and the planes: disjoint, but for state_in == state_out
    Range r[5];
    int n = 0;
    r[n++] = range_of(work, SAH_EXPOSURE_WORK_BYTES);
    r[n++] = range_of(state_out, sizeof(sah_exposure_state));
    if (history && (const void*)state_in != (const void*)state_out) r[n++] = range_of(state_in, sizeof(sah_exposure_state));
    const int buffers = n;
    r[n++] = range_of(scene);
    if (exposed_out) r[n++] = range_of(exposed_out);
    for (int i = 0; i < buffers; i++)
        for (int j = i + 1; j < n; j++)
            if (overlap(r[i], r[j])) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: work, the states and the planes must not overlap");
    sah::ExposureArgs a{};
    a.scene = parg(scene), a.out = parg(exposed_out);
    a.W = scene->width, a.H = scene->height;
    a.work = static_cast<uint32_t*>(work);
    a.state_in = history ? state_in : nullptr, a.state_out = state_out;
    a.key = s.key, a.low_fraction = s.low_fraction, a.high_fraction = s.high_fraction, a.min_exposure = s.min_exposure, a.max_exposure = s.max_exposure;
    a.adaptation = s.adaptation, a.history = history;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_exposure_meter(a, exposed_out != nullptr, s.max_workgroups, ctx->stream));
    return SAH_OK;
}

extern "C" int sah_exposure_apply(sah_ctx* ctx, const sah_plane* scene, const sah_exposure_state* state, const sah_plane* out, uint32_t row_begin,
                                  uint32_t row_end) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!state) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_apply: state is null");
    const struct {
        const sah_plane* p;
        const char* what;
    } planes[2] = {{scene, "scene"}, {out, "out"}};
    for (const auto& pl : planes)
        if (const int rc = plane_status(pl.p); rc != SAH_OK)
            return fail(ctx, rc, "exposure_apply: %s must be an R16G16B16A16_SFLOAT plane, 4-byte aligned, with a pitch of at least a row", pl.what);
    if (const char* why = pair_problem(scene, out)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_apply: %s", why);
    const uint32_t h = scene->height;
    if (row_begin == 0 && row_end == 0) row_end = h;
    if (row_end > h || row_begin > row_end) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_apply: bad row range");
    if ((uintptr_t)state % 4) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_apply: state must be 4-byte aligned");
    const Range st = range_of(state, sizeof(sah_exposure_state));
    if (overlap(st, range_of(scene)) || overlap(st, range_of(out))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_apply: state overlaps a plane");
    sah::ExposureArgs a{};
    a.scene = parg(scene), a.out = parg(out);
    a.W = scene->width, a.H = h, a.row_begin = row_begin, a.row_end = row_end;
    a.state_in = state;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_exposure_apply(a, ctx->stream));
    return SAH_OK;
}
