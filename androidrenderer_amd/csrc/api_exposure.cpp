// C ABI: histogram auto-exposure (include/sah_exposure.h; kernels in exposure.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_exposure.h"
#include "ctx.hpp"
#include "launch.hpp"

namespace {
// scene and a target of it: one extent below 2^32 texels; the target is the scene's plane itself or disjoint from it
const char* pair_problem(const sah_plane* scene, const sah_plane* target) {
    if (texel_count_too_large(scene->width, scene->height)) return "2^32 texels or more";
    if (!target) return nullptr;
    if (target->width != scene->width || target->height != scene->height) return "the planes must have one extent";
    const bool same = target->ptr == scene->ptr && target->row_pitch_bytes == scene->row_pitch_bytes;
    if (!same && overlaps(byte_range(scene), byte_range(target))) return "the target overlaps the scene without being the same plane";
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
    const PlaneSpec planes[2] = {{scene, SAH_FORMAT_R16G16B16A16_SFLOAT, "scene (R16G16B16A16_SFLOAT)"},
                                 {exposed_out, SAH_FORMAT_R16G16B16A16_SFLOAT, "exposed_out (R16G16B16A16_SFLOAT)"}};
    if (const int rc = check_planes(ctx, "exposure_meter", planes, exposed_out ? 2 : 1); rc != SAH_OK) return rc;
    if (const char* why = pair_problem(scene, exposed_out)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: %s", why);
    if (!positive_finite(s.key) || !positive_finite(s.min_exposure) || !positive_finite(s.max_exposure) || s.min_exposure > s.max_exposure)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: key, min_exposure and max_exposure must be finite and positive, min <= max");
    if (!(s.low_fraction >= 0.0f && s.low_fraction < s.high_fraction && s.high_fraction <= 1.0f))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: the fractions must be 0 <= low < high <= 1");
    if (!(s.adaptation > 0.0f && s.adaptation <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: adaptation must be in (0, 1]");
    if (((uintptr_t)work % 4) || ((uintptr_t)state_out % 4) || (history && ((uintptr_t)state_in % 4)))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: work and the states must be 4-byte aligned");
    // work, state_out, state_in and the planes: disjoint, but for state_in == state_out
    ByteRange r[5];
    int n = 0;
    r[n++] = byte_range(work, SAH_EXPOSURE_WORK_BYTES);
    r[n++] = byte_range(state_out, sizeof(sah_exposure_state));
    if (history && (const void*)state_in != (const void*)state_out) r[n++] = byte_range(state_in, sizeof(sah_exposure_state));
    const int buffers = n;
    r[n++] = byte_range(scene);
    if (exposed_out) r[n++] = byte_range(exposed_out);
    for (int i = 0; i < buffers; i++)
        for (int j = i + 1; j < n; j++)
            if (overlaps(r[i], r[j])) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_meter: work, the states and the planes must not overlap");
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
    const PlaneSpec planes[2] = {{scene, SAH_FORMAT_R16G16B16A16_SFLOAT, "scene (R16G16B16A16_SFLOAT)"}, {out, SAH_FORMAT_R16G16B16A16_SFLOAT, "out (R16G16B16A16_SFLOAT)"}};
    if (const int rc = check_planes(ctx, "exposure_apply", planes, 2); rc != SAH_OK) return rc;
    if (const char* why = pair_problem(scene, out)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_apply: %s", why);
    const uint32_t h = scene->height;
    if (!resolve_rows(&row_begin, &row_end, h)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_apply: bad row range");
    if ((uintptr_t)state % 4) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_apply: state must be 4-byte aligned");
    const ByteRange st = byte_range(state, sizeof(sah_exposure_state));
    if (overlaps(st, byte_range(scene)) || overlaps(st, byte_range(out))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "exposure_apply: state overlaps a plane");
    sah::ExposureArgs a{};
    a.scene = parg(scene), a.out = parg(out);
    a.W = scene->width, a.H = h, a.row_begin = row_begin, a.row_end = row_end;
    a.state_in = state;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_exposure_apply(a, ctx->stream));
    return SAH_OK;
}
