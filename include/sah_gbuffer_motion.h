/* sah_gbuffer_motion.h — the G-buffer pass and the motion-vectors pass in one call, with one rasteriser set-up.
 *
 * A frame that needs motion vectors (an anti-aliasing mode or an upscaler is on: RenderCore/render/scene_renderer.cpp:308-316) calls
 * sah_gbuffer_render and then sah_motion_vectors_render for the same scene and view.  The second call repeats all the first one did
 * before its tile kernel — the vertex stage, clipping, set-up, binning, the read-back of the rasteriser's counters — to arrive at the
 * numbers the first call already had in scratch memory.  This call does that work once.  Same conventions as sah_hip.h and
 * sah_motion_vectors.h (this header includes both); DESIGN.md §5n.
 */
#ifndef SAH_GBUFFER_MOTION_H
#define SAH_GBUFFER_MOTION_H

#include "sah_hip.h"
#include "sah_motion_vectors.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The call IS the composition: after it the five planes of `out`, `motion_vectors` and `stats` hold, bit for bit, what
 *
 *     sah_gbuffer_render(ctx, scene, view, out, stats);
 *     sah_motion_vectors_render(ctx, scene, view, &out->depth, motion_vectors, NULL);
 *
 * leave there: padding bytes of pitched planes are not touched, non-finite motion values are stored as they come, a SOLID fragment at
 * depth exactly 0 over a cleared texel gets its motion vector although the G-buffer pass drops it, and a pixel a CUTOUT fragment wins
 * holds the motion vector of a SOLID fragment of bit-equal depth if there is one, (0, 0) otherwise.
 *
 * One exception, for a malformed scene: a SOLID primitive whose `material` is not below num_materials is dropped by the G-buffer
 * pass's range check (stats[2]) and with it from the shared records, so it gets no motion vectors either; the stand-alone motion
 * pass, which reads no materials, would draw it.
 *
 * stats: device, SAH_RASTER_STATS_WORDS words, or NULL: the eight words of sah_gbuffer_render.  The statistics of the stand-alone
 * motion pass (in which CUTOUT triangles count as culled) are not reported: that pass's set-up is the work this call does not do.
 *
 * Arguments are those of the two calls with `depth` = &out->depth, checked before anything is launched, the G-buffer call's first:
 * SAH_ERR_INVALID_ARGUMENT for a NULL pointer, a scene without the arrays sah_gbuffer_render needs, or an extent outside 1..8192;
 * SAH_ERR_UNSUPPORTED_FORMAT for a plane of `out` with the wrong format, extent or alignment; SAH_ERR_INVALID_ARGUMENT for a
 * `motion_vectors` that is not an R16G16_SFLOAT plane of the depth plane's extent, 4-byte aligned, its pitch a multiple of 4 and at
 * least a row.  `motion_vectors` must not overlap a plane of `out`: the call does not check it (planes interleaved row by row in one
 * allocation are legitimate and look the same to a cheap test), and the result of an overlap is undefined.  Failures found on the
 * device are sah_gbuffer_render's: invalid texture slots or bindings (SAH_ERR_INVALID_ARGUMENT), more than 2^28 triangles
 * (SAH_ERR_UNSUPPORTED).
 *
 * Runs on the context's stream with the host synchronisation of sah_gbuffer_render: one read-back of the rasteriser's counters per
 * attempt, the whole fused pass repeated when a scratch buffer was guessed too small (sah_debug_raster_last_pass reports it).  Like
 * the two calls it replaces it cannot be recorded under stream capture, and it moves no cache and no epoch of the context. */
int sah_gbuffer_motion_render(sah_ctx* ctx, const sah_scene_geometry* scene, const sah_view_data* view, const sah_gbuffer* out,
                              const sah_plane* motion_vectors, uint32_t* stats);

#ifdef __cplusplus
}
#endif

#endif /* SAH_GBUFFER_MOTION_H */
