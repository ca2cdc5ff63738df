/* sah_motion_vectors.h — the motion-vectors pass: screen-space motion of solid geometry between the last frame and this one.
 *
 * SceneRenderer::render runs it right after the depth pre-pass when an anti-aliasing mode or an upscaler needs it
 * (RenderCore/render/scene_renderer.cpp:308-316, `needs_motion_vectors`); shaders in RenderCore/shaders/motion_vectors.  Same
 * conventions as sah_hip.h (this header includes it); the rasterisation rules are those of sah_gbuffer_render.
 */
#ifndef SAH_MOTION_VECTORS_H
#define SAH_MOTION_VECTORS_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MotionVectorsPhase::render — RenderCore/render/phase/motion_vectors_phase.cpp:55-103.
 *
 * Clear      every texel of `motion_vectors` is (0, 0) unless a fragment below writes it (:90-92).
 * Draws      scene.draw_opaque: the SOLID primitives only, in list order, back faces culled by the rule of sah_gbuffer_render; CUTOUT
 *            primitives are not drawn.  The reference draws what its visibility list holds, and that list is all ones
 *            (hi_z_culling.comp:147-162 sets this_frame_visible = 1 on every path), so drawing every SOLID primitive is faithful; the
 *            order of its atomic compaction is pinned to list order, as in sah_gbuffer_render.
 * Vertex     motion_vectors.vert.slang:27-31: world = model * p, clip = projection * (view * world) with exactly the arithmetic of
 *            the G-buffer pass's vertex stage, so the window-space triangles, the clipping and the fragment depths are the numbers
 *            that pass produces; prev = last_frame_projection * (last_frame_view * world) by the same matrix-vector rule, and the
 *            varying is (prev.x, prev.y, prev.w) in fp32.  The same `model` serves both frames (the reference's quirk: objects have
 *            no motion of their own).
 * Depth      compare EQUAL, no depth write, no blending (:20-25): a fragment passes iff its depth — the G-buffer pass's depth rule,
 *            clamped to [0, 1] as there — is bit-equal to its texel of `depth`.  Among the passing fragments of a pixel the last in
 *            draw order stays.
 * Fragment   motion_vectors_opaque.frag.slang:18-24, every operator rounded on its own in fp32, no contraction: the varying is
 *            v = (l0 * a0 + l1 * a1) + l2 * a2 with the perspective-correct weights the G-buffer pass applies to its float2 texcoord
 *            (for a clipped triangle through the barycentrics of the clipped vertices in the input triangle);
 *            ndc = v.xy / v.z (two divisions); uv = ndc * 0.5 + 0.5; p = uv * view->render_resolution;
 *            mv = p - (px + 0.5, py + 0.5); stored as two halfs, round to nearest even, overflow to infinity.  Non-finite results are
 *            stored as they come (the shader has no guard).
 *
 * depth: D32_SFLOAT, read only (what sah_gbuffer_render wrote for the same scene and view); motion_vectors: R16G16_SFLOAT of the same
 * extent (r.MotionVectors.FullRes, which only changes the target's extent, is not supported); both 4-byte aligned with pitches that
 * are multiples of 4.  scene->vertex_data, materials and textures are not read and may be NULL.  stats: device,
 * SAH_RASTER_STATS_WORDS words, or NULL; CUTOUT triangles count as culled.
 *
 * SAH_ERR_INVALID_ARGUMENT, before anything is launched: a NULL pointer, a wrong format, differing or unsupported extents, a pitch
 * smaller than a row.  Index and primitive ranges follow the rule of sah_gbuffer_render: a draw that points outside the index or
 * vertex arrays is dropped, never dereferenced (stats[2]).
 *
 * Runs on the context's stream with the host synchronisation of sah_gbuffer_render (one read-back of the rasteriser's counters per
 * call); leaves `depth`, and every cache and epoch of the context, untouched. */
int sah_motion_vectors_render(sah_ctx* ctx, const sah_scene_geometry* scene, const sah_view_data* view, const sah_plane* depth,
                              const sah_plane* motion_vectors, uint32_t* stats);

#ifdef __cplusplus
}
#endif

#endif /* SAH_MOTION_VECTORS_H */
