/* sah_lpv_gv.h — the LPV geometry volume (GV): its two producers and the propagation that reads it.
 *
 * LightPropagationVolume with r.GI.LPV.GvBuildMode = DepthBuffers (the reference's default,
 * RenderCore/render/gi/light_propagation_volume.cpp:49-53) builds the GV every frame from the RSM depth of every cascade
 * (inject_indirect_sun_light, :689-693) and from the scene depth (post_render, :238-247); lpv_propagate.comp.slang:104-114 then
 * attenuates each face's flux by the GV when use_gv is set (the reference's host passes use_gv = 0, :975).  Same conventions as
 * sah_hip.h (this header includes it).  The GV is an RGBA16F volume of (32 * num_cascades) x 32 x 32 texels, zeroed by sah_lpv_clear's
 * `geometry` argument; it is not an input of sah_lighting, so none of these calls touches the Lighting pass's LPV gather copy.
 *
 * Blend (both injections): per channel dst = max(dst, RN16(src)) over whatever the GV held, in the total order of the
 * half bit patterns  -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN  (so -0 < +0, a NaN already in the GV with the sign bit clear stays,
 * one with the sign bit set is replaced by any value).  A NaN source channel leaves its channel unchanged.  The result is independent
 * of the order of the points.
 *
 * Point to texel (both injections): the rule of sah_lpv_inject_vpls — x_f = ndc_x * W / 2 + W / 2 (likewise y), floor, kept when in
 * [0, W) x [0, H) and the layer float in (-1, D); W, H, D are the GV's extents; non-finite positions are dropped.
 */
#ifndef SAH_LPV_GV_H
#define SAH_LPV_GV_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* "Inject RSM depth into GV" — gv_injection.{vert,frag} for cascades [first_cascade, first_cascade + cascade_count) of num_cascades, in
 * one launch (MAX does not depend on the order, so this equals one call per cascade).  Vertex i of a cascade c reads RSM texel
 * (x, y) = (2i mod res, 2i div res) for i < res_x * res_y (only even columns; rows >= res_y are dropped) through the default sampler
 * (NEAREST, REPEAT) at ((0.5 + x) / res, (0.5 + y) / res), layer c; NDC (x / res * 2 - 1, y / res * 2 - 1, depth, 1) through
 * inverse_projection = I, / w, inverse_view = cascades[c].inverse_rsm_vp, then world_to_cascade; dropped when a cascade coordinate of
 * xyz is outside [0, 1]; then + 0.5 / 32 on all four components, x = (x + c) / num_cascades, gl_Position = (x * 2 - 1, y * 2 - 1, 0, 1),
 * layer int(z * 32).  The value is dir_to_cosine_lobe(normal) of the UNORM normal as read (no * 2 - 1), in fp32.
 * rsm->normals: R8G8B8A8_UNORM, rsm->depth: D16_UNORM, equal extents, at least first_cascade + cascade_count layers (rsm->flux is not
 * read).  num_cascades in [1, 4]. */
int sah_lpv_inject_rsm_gv(sah_ctx* ctx, const sah_rsm_targets* rsm, const sah_lpv_cascade_matrices* cascades, uint32_t first_cascade,
                          uint32_t cascade_count, uint32_t num_cascades, const sah_volume* geometry);

/* "Inject scene depth into GV" — inject_scene_depth_into_gv.{vert,geom,frag}: vertices i < W * H / 4 (uint32: only the first quarter of
 * the rows), texel (i mod W, i div W) read with texelFetch; position from screenspace ((x + 0.5) / W, (y + 0.5) / H) * 2 - 1 and the
 * depth through view->inverse_projection, / w, view->inverse_view (sky pixels, depth 0, give w = 0 and are dropped); the normal is not
 * normalised.  Per cascade c (the geometry shader): world_to_cascade, dropped outside [0, 1], else gl_Position = ((x + c) / num_cascades,
 * y, 0, 1) — no * 2 - 1 and no half-cell offset, so points land in the upper half of x and y — layer int(z * 32).
 * depth: D32_SFLOAT, normals: R16G16B16A16_SFLOAT, equal extents. */
int sah_lpv_inject_scene_gv(sah_ctx* ctx, const sah_plane* depth, const sah_plane* normals, const sah_view_data* view,
                            const sah_lpv_cascade_matrices* cascades, uint32_t num_cascades, const sah_volume* geometry);

/* sah_lpv_propagate with use_gv = 1.  geometry == NULL: exactly sah_lpv_propagate (gather-copy emission and epoch rules included).
 * Otherwise each face's contribution is ((sa * m) * lobe) * factor with, in half,
 *   factor = 1 - clamp(gv.x * sh.x + abs(dot(gv.yzw, sh.yzw)), 0, 1)      (clamp = min(max(x, 0), 1), IEEE maxNum / minNum: NaN -> 0)
 * where gv = the GV sampled (LINEAR, CLAMP_TO_BORDER transparent black; the weighted sum of DESIGN.md §3 in fp32, rounded to half4) at
 * ((n.x / 32 + 0.5 / 32) + cascade) / 4 — a literal 4: an exact texel centre with four cascades only — and n.yz / 32 + 0.5 / 32 for the
 * neighbour cell n.  The GV must not alias the colour volumes. */
int sah_lpv_propagate_gv(sah_ctx* ctx, const sah_volume a_rgb[3], const sah_volume b_rgb[3], const sah_volume* geometry, uint32_t num_cascades,
                         uint32_t steps);

#ifdef __cplusplus
}
#endif

#endif /* SAH_LPV_GV_H */
