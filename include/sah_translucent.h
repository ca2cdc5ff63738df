/* sah_translucent.h — alpha-blended geometry over the lit scene: the primitives the reference's importer files under
 * TransparencyMode::Translucent (model_import/gltf_model.cpp:193-197, render/basic_pbr_material.hpp:14-18) and its scene keeps in
 * `translucent_primitives` for `draw_transparent()` (render/render_scene.cpp:66-67, 234-236).  The reference never finished the pipeline that
 * would draw them; its blend state is still there, commented out (render/material_pipelines.cpp:137-153: SRC_ALPHA / ONE_MINUS_SRC_ALPHA,
 * colour and alpha alike).  Every rule below is therefore ABI-defined.  The rules are chosen so that no new shading arithmetic exists: a
 * fragment is rasterised by the G-buffer pass's own stages and lit by sah_lighting's own restatement; what is new is the peel that brings
 * every fragment of a pixel to the blend in draw order.  Restated as a composition of sah_gbuffer_render + sah_lighting by
 * tests/translucent_ref.py and pinned bit for bit by tests/golden/translucent_96x54.npz.  Off by default everywhere: nothing in the library,
 * in include/sah_host.hpp or in androidrenderer_amd/frame.py runs it unless the caller asks.  Its place is after sah_lighting (and after
 * sah_ssr, where used) and before sah_sun_shafts and the anti-aliasing.  Not part of sah_chain_*.  Same conventions as sah_hip.h (this header
 * includes it).
 *
 * The other entry points are unchanged: they do not look at a primitive's type beyond SOLID / CUTOUT, so a type-2 primitive handed to
 * sah_gbuffer_render, sah_shadow_render, sah_rsm_render or sah_rt_build is an opaque two-sided wall there, as it always was.  A caller hands
 * them the scene without its type-2 primitives and hands this call the scene that has them (this call draws nothing else of it);
 * androidrenderer_amd.mesh.split_translucent makes the two.
 *
 * Host behaviour is sah_gbuffer_render's: the rasteriser scratch of the context, regrown the same way, and one read-back of the counters
 * (a host synchronisation) per attempt.  Not capturable.
 */
#ifndef SAH_TRANSLUCENT_H
#define SAH_TRANSLUCENT_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_PRIMITIVE_TYPE_TRANSLUCENT 2 /* TransparencyMode::Translucent, PRIMITIVE_TYPE_TRANSPARENT of shared/primitive_data.hpp:8 */

typedef struct sah_translucent_desc {
    const sah_lighting_desc* lighting; /* the frame's own Lighting descriptor: `lit` is read and written, gbuffer->depth is tested against */
    const sah_scene_geometry* scene;   /* only its primitives of type SAH_PRIMITIVE_TYPE_TRANSLUCENT are drawn */
    uint32_t* stats;                   /* device, SAH_RASTER_STATS_WORDS words or NULL; words 0-4 as in the other passes, counted over the
                                          translucent triangles; 5 and 6 are 0 (no list is cut); word 7 = most fragments blended at one pixel */
} sah_translucent_desc;

/* Blends the translucent primitives of desc->scene into desc->lighting->lit (all ABI-defined).
 *
 * Geometry    The vertex stage, clipping, fanning, snapping, fill rule and fragment depth of sah_gbuffer_render, as they are, with
 *             desc->lighting->view as the view.  No face culling, as for CUTOUT; the normal is not flipped for a back face.  No alpha test.
 *             Non-finite and out-of-range triangles are dropped and counted as in the other passes.
 * Depth test  A fragment at pixel q with depth z takes part iff z > depth[q] in fp32 (reverse-Z GREATER, strict); a NaN compares false; a
 *             sky texel (0) lets every z > 0 through.  Nothing is written to the depth plane.
 * Order       Per pixel, fragments are blended in draw order: translucent primitives in list order, triangles in index order, fan pieces
 *             of a clipped triangle in fan order (the rasteriser's sequence number, counted over the translucent triangles alone).  The
 *             caller sorts the primitives back to front, as draw_transparent() would be fed.  The order in which bin entries or workgroups
 *             arrive does not show in the result.
 * Fragment    The five values sah_gbuffer_render's fragment stage would write for this fragment — colour with its alpha code, normals,
 * texel       data, emission, and z — in the G-buffer's formats, with the same texture sampling and derivatives.
 * Fragment    S, four halfs: what sah_lighting(ctx, desc->lighting) writes at q for a G-buffer whose texel at q is that fragment texel,
 * colour      with an AO of 1 and no sky (z > 0: a fragment is a surface).  Supported: sun off or CSM, GI none or LPV, with the flags of
 *             sah_lighting (SAH_LIGHTING_QUIRK_SUN_BLEND included).  SAH_ERR_UNSUPPORTED, before any launch, for the RT sun mode (there
 *             is no mask for a fragment), GI kinds CACHE and RTGI, and a non-empty light list.
 * Blend       a = the UNORM8-to-float table value of the fragment's alpha code.  A fragment with code 0 is skipped.  Otherwise, per channel
 *             of all four, with D the half now at q: (S * a) + (D * (1 - a)), every operator rounded in fp32, no fma, stored as a half by
 *             the conversion Lighting's own store uses (round to nearest even).  Each blend is rounded to the attachment's format, the
 *             convention sah_lpv_inject_vpls follows for its additive blend.
 * Rows        row_begin / row_end of desc->lighting limit the pixels written, (0, 0) = all rows.  A sharded frame equals the unsharded one.
 * Nothing to  A tile that no translucent triangle touches reads and writes no plane: with no type-2 primitive, or none on screen, `lit`
 * draw        keeps its bytes.  Departure from "no tile work is launched": the primitives are in device memory and the call's one
 *             read-back comes after its launches, so the tile grid is always launched; a workgroup whose bin list is empty returns at
 *             once.  Statistics word 4 (bin entries) is then 0.
 * Cost        One workgroup per 64 x 64 tile walks the tile's whole bin list once per layer: a tile costs (list length) x (deepest
 *             pixel).  Lists are not cut into parts, as the opaque passes cut theirs: a peel cannot be merged across workgroups.
 *
 * Before anything is launched: everything sah_lighting and sah_gbuffer_render refuse, with their codes (for the scene, the extent up to
 * 8192, the formats and the alignment of the depth plane and of lit); SAH_ERR_INVALID_ARGUMENT for a NULL desc, lighting or scene and for a
 * `lit` that overlaps a plane of the G-buffer; `lit` of another extent than the depth plane is SAH_ERR_UNSUPPORTED_FORMAT, sah_lighting's
 * code for it.  A bad texture table fails the call as in sah_gbuffer_render, and `lit` keeps its bytes.
 *
 * Not built: per-pixel sorting or any other order-independent transparency, refraction, translucent shadows (coloured or not), motion
 * vectors for translucent surfaces, translucent surfaces in the ray-traced passes, sah_chain_* integration, consumption by sah_lighting_vrs. */
int sah_translucent_render(sah_ctx* ctx, const sah_translucent_desc* desc);

#ifdef __cplusplus
}
#endif

#endif /* SAH_TRANSLUCENT_H */
