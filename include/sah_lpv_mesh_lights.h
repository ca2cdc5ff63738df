/* sah_lpv_mesh_lights.h — LPV mesh lights: emissive surfaces turned into VPL clouds and added to the LPV volumes.
 *
 * LightPropagationVolume::pre_render (RenderCore/render/gi/light_propagation_volume.cpp:223-236) runs, after the sun injection,
 * inject_emissive_point_clouds (:787-834) when r.GI.LPV.MeshLight.Enable is set (:73-75, default 1).  Three stages:
 *   1. load time, host: MeshStorage::add_mesh -> generate_surface_point_cloud (RenderCore/render/mesh_storage.cpp:140-166, 246-319,
 *      interpolate_vertex :321-370, find_reservoir :418-450)                                   -> sah_mesh_point_cloud
 *   2. once per new emissive primitive: RenderScene::generate_vpls_for_primitive (RenderCore/render/render_scene.cpp:255-310) with
 *      RenderCore/shaders/util/emissive_point_cloud.comp                                       -> sah_lpv_emissive_vpls
 *   3. every frame, per cascade: get_primitives_in_bounds (render_scene.cpp:136-160) and one vpl_injection.{vert,frag} point draw
 *      per selected emissive cloud, blended ONE / ONE into the A volumes                       -> sah_lpv_inject_emissive
 * Same conventions as sah_hip.h (this header includes it).  Two defects of the reference are fixed here, so that the result is a
 * function of the input:
 *   - the seed: generate_surface_point_cloud seeds std::default_random_engine from std::random_device (mesh_storage.cpp:292-293); here
 *     the caller passes the seed.
 *   - the push constants: the host passes 5 fields (render_scene.cpp:267-273), emissive_point_cloud.comp declares 6 (:34-41), so the
 *     shipped shader reads its buffers from the wrong offsets.  This ABI defines what the shader evidently means (stage 2 below).
 */
#ifndef SAH_LPV_MESH_LIGHTS_H
#define SAH_LPV_MESH_LIGHTS_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sah_mesh_point_cloud flags */
#define SAH_POINT_CLOUD_ON_SURFACE 1u /* weights b / ((b.x + b.y) + b.z), no / 3: the points lie on the triangles (default: the quirk) */

/* Point cloud of one mesh, on the host (no context, no GPU).  The mesh is the index range indices[first_index, first_index + index_count)
 * (index_count a multiple of 3, first_index + index_count <= num_indices), vertex v of a triangle being positions[3 * (v + vertex_offset)]
 * and vertex_data[v + vertex_offset] (each in [0, num_vertices)).  All pointers are HOST pointers.
 *   area       per triangle: length(cross(p0 - p1, p0 - p2)) in fp32 (cross as glm, length = sqrt((x*x + y*y) + z*z)), then / 2.0 in
 *              double; summed in double in triangle order; each divided by the total, then prefix-summed, in double.
 *   count      min(ceil(total / 0.1), 65536) in double; 0 when the total is 0 or not finite.
 *   engine     minstd_rand0 (x <- 16807 x mod 2^31 - 1) seeded with `seed` the standard's way: seed mod (2^31 - 1), 0 -> 1.
 *   uniform    libstdc++'s uniform_real_distribution<double>{0, 1} over that engine: two draws x1, x2, in double
 *              u = ((x1 - 1) + (x2 - 1) * R) / (R * R), R = 2147483646; a result >= 1 becomes the double below 1.
 *   sample     per point, in this order: u (the reservoir), then u1, u2, u3 converted to float, b = glm::normalize(vec3{u1, u2, u3}) =
 *              v * (1 / sqrt((x*x + y*y) + z*z)) in fp32 (glm 1.0.0).
 *   reservoir  the first triangle whose prefix is > u, the last triangle when none is.  That is find_reservoir on every input where
 *              find_reservoir terminates; a zero-area triangle is never chosen unless it is the last one.
 *   vertex     interpolate_vertex: for position, normal, tangent, texcoord and colour ((a0 * w.x + a1 * w.y) + a2 * w.z) / 3 in fp32,
 *              w = b (its quirk: b is unit length, not summing to one, so points land 1/3 .. 0.58 of the way from the mesh origin),
 *              or w = b / ((b.x + b.y) + b.z) and no / 3 with SAH_POINT_CLOUD_ON_SURFACE.  Colour: unpackUnorm4x8 (byte * (1 / 255.0f)),
 *              packUnorm4x8 = round(clamp(c, 0, 1) * 255) with halves away from zero (a NaN channel gives 0).
 * bounds_min / bounds_max (may be NULL): the per-axis minimum and maximum of the referenced positions (glTF's accessor min / max; NaN
 * coordinates are ignored; +inf / -inf for an empty range).  *out_count always receives the number of points.  out_positions
 * (3 floats per point) and out_points may both be NULL with capacity 0 (a size query); otherwise both are needed and capacity must hold
 * the count, else SAH_ERR_INVALID_ARGUMENT and nothing is written but the count and the bounds. */
int sah_mesh_point_cloud(const float* positions, const sah_vertex_data* vertex_data, uint32_t num_vertices, const uint32_t* indices,
                         uint32_t num_indices, uint32_t first_index, uint32_t index_count, int32_t vertex_offset, uint64_t seed, uint32_t flags,
                         float* out_positions, sah_vertex_data* out_points, uint32_t capacity, uint32_t* out_count, float bounds_min[3],
                         float bounds_max[3]);

/* sah_lpv_emissive_vpls flags */
#define SAH_EMISSIVE_MATERIAL_ZERO 1u /* read materials[0], the shipped shader's literal (emissive_point_cloud.comp:64, a TODO) */

/* emissive_point_cloud.comp, one invocation per point: VPL i of out_vpls (DEVICE, num_points entries) from point i of the cloud
 * (positions: 3 floats per point, points: sah_vertex_data; DEVICE).
 *   material   scene->materials[scene->primitives[primitive_index].material] — the primitive's own, which is what the host's
 *              primitive_index is for — or materials[0] with SAH_EMISSIVE_MATERIAL_ZERO.  A material index at or beyond num_materials
 *              gives colour 0 (a VPL the injection drops).
 *   colour     emission_sample * emission_factor (fp32 per channel); the sample is the material's emission texture read with an
 *              explicit level of detail 0 (a compute shader's texture() has no derivatives): SampleLevel as sah_texture fixes it for
 *              the ray-tracing stages — lambda = 0 + sampler.mip_lod_bias, clamped to [min_lod, max_lod], then filter, level and tau.
 *              SAH_TEXTURE_NONE, no texture table, or a slot outside it: the material's constant emission_texel.
 *   position   primitive.model * (p, 1), each row ((m0 x + m1 y) + m2 z) + m3 in fp32 (the rasteriser's vertex stage); the NORMAL is the
 *              point's own, untransformed (as the shader does).
 *   packing    PackedVPL: halfs rounded to nearest even (inf and NaN stay inf and NaN), normal packSnorm4x8(vec4(n, 0)) as
 *              sah_lpv_extract_vpls packs it (clamp, * 127, round half to even). */
int sah_lpv_emissive_vpls(sah_ctx* ctx, const sah_scene_geometry* scene, uint32_t primitive_index, const float* positions,
                          const sah_vertex_data* points, uint32_t num_points, uint32_t flags, sah_packed_vpl* out_vpls);

/* One primitive's cloud, as sah_lpv_inject_emissive takes it: its VPL list (DEVICE, from sah_lpv_emissive_vpls), the primitive and the
 * bounds of its mesh (sah_mesh_point_cloud, mesh space). */
typedef struct sah_emissive_cloud {
    const sah_packed_vpl* vpls;
    uint32_t count;
    uint32_t primitive;
    float bounds_min[3], bounds_max[3];
} sah_emissive_cloud;

/* LightPropagationVolume cascade bounds (light_propagation_volume.cpp:514-515): snapped offset -+ size / 2. */
typedef struct sah_lpv_cascade_bounds {
    float min_bounds[3], max_bounds[3];
} sah_lpv_cascade_bounds;

/* Largest number of (cascade, light) entries one sah_lpv_inject_emissive call takes: the sum of the clouds' counts times num_cascades.
 * The call needs about 72 bytes of context scratch per entry (grown, never shrunk). */
#define SAH_LPV_EMISSIVE_MAX_ENTRIES (1u << 24)

/* inject_emissive_point_clouds: for cascade c = 0 .. num_cascades - 1, then cloud k in array order (the façade passes them in ascending
 * primitive index, the reference's list order), then point p, the VPL clouds[k].vpls[p] goes through the vertex and fragment stage of
 * sah_lpv_inject_vpls with cascade index c — cells of a neighbour cascade, the length(normalize(n)) < 1 discard and the saturation boost
 * included — when cloud k is SELECTED for cascade c:
 *   the primitive scene->primitives[clouds[k].primitive] is SOLID (get_primitives_in_bounds walks solid_primitives only), its material
 *   (index < num_materials) is emissive — length(emission_factor.rgb) > 0 in fp32, or an emission texture slot != SAH_TEXTURE_NONE when the
 *   scene has a texture table (gltf_model.cpp:210-213, 264-276) — and its box strictly overlaps the cascade's: with lo = model * (bounds_min,
 *   1) and hi = model * (bounds_max, 1) (two corners only, in the rasteriser's row order, NOT re-sorted: a rotated or mirrored model can
 *   give lo > hi), per axis bounds[c].min_bounds < hi && bounds[c].max_bounds > lo (Box::overlaps, RenderCore/core/box.cpp).
 * The selection is evaluated on the device from scene->primitives / materials / material_textures.
 * Result: exactly what sah_lpv_inject_vpls(the concatenation of the selected clouds' lists, cascade c) for c = 0, 1, ... in sequence
 * produces: the lights of one cell are added onto the texel's current value in (cascade, cloud, point) order, each sum rounded to half.
 * No capacity limit below SAH_LPV_EMISSIVE_MAX_ENTRIES (more: SAH_ERR_INVALID_ARGUMENT).  No host synchronisation: the grids are sized from
 * the host-known counts.  The volumes: three RGBA16F volumes of one extent with at most 2^17 texels ((32 * num_cascades) x 32 x 32 for
 * up to four cascades), 8-byte aligned.  clouds, cascades and bounds are HOST arrays. */
int sah_lpv_inject_emissive(sah_ctx* ctx, const sah_scene_geometry* scene, const sah_emissive_cloud* clouds, uint32_t num_clouds,
                            const sah_lpv_cascade_matrices* cascades, const sah_lpv_cascade_bounds* bounds, uint32_t num_cascades,
                            const sah_volume a_rgb[3]);

#ifdef __cplusplus
}
#endif

#endif /* SAH_LPV_MESH_LIGHTS_H */
