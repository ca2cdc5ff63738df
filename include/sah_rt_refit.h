/* sah_rt_refit.h — refit of the acceleration structure: the per-frame operation for a scene whose objects move.  Same conventions as
 * sah_hip.h (this header includes it).
 *
 * The reference has no update path of its own: it commits its TLAS every frame over BLASes that persist
 * (RenderCore/render/raytracing_scene.cpp:50-170) — instance transforms change, topology does not.  This library folds both levels into
 * one structure (sah_hip.h "ray tracing"), so the equivalent is: keep the triangles and their order, refresh the coordinates.  The whole
 * entry is builder-owned, like the row windows of sah_rt_set_rows; what it fixes is marked "ABI-defined".
 *
 * The padded triangle box is part of the DEFINITION of a hit (sah_hip.h "hit"), and slab() is monotone under box inclusion: a ray's
 * result through a refit structure equals its result through a rebuilt one and equals testing every triangle.  What a stale order costs
 * is boxes met per ray, never a result.
 */
#ifndef SAH_RT_REFIT_H
#define SAH_RT_REFIT_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Refreshes the context's acceleration structure from `scene` as its arrays are NOW (ABI-defined throughout).
 *
 * May have changed since the sah_rt_build (or sah_rt_refit) that made the structure: the contents of vertex_positions; every
 *            primitives[i].model; vertex_data, materials and textures (the hit stages read them at trace time); every address in `scene`
 *            (the context traces against the arrays of the last build OR refit, which must stay valid while rays are traced).
 * Promised unchanged: num_primitives, num_vertices, num_indices — checked on the host: a mismatch is SAH_ERR_INVALID_ARGUMENT before
 *            anything is launched, the structure untouched —; the index array; each primitive's first_index, index_count, vertex_offset
 *            and type — not checked, but no read leaves the arrays: indices are bounds-checked as the build does, and a triangle whose
 *            indices no longer resolve is treated like a non-finite one.
 * Triangles  position i of the structure keeps its (primitive, triangle-in-primitive, CUTOUT flag).  Its vertices become
 *            model * (p_k, 1), each row ((m0 x + m1 y) + m2 z) + m3 in fp32: the build's arithmetic, bit for bit.
 * Absent     a triangle with a non-finite new world vertex is ABSENT: no ray hits it, its stored vertices are zeros, it does not enter
 *            S.  A later refit with finite vertices brings it back.  A triangle the BUILD left out stays out: a refit equals a rebuild
 *            exactly when the build's left-out set would be left out again (always so for index faults).
 * pad        S * 2^-16 with S the largest |coordinate| over the present triangles of THIS refit.  S is reduced on the device and read
 *            from device memory by the kernel that makes the boxes; it never reaches the host.
 * Boxes      a triangle's box is [min_k v_k - pad, max_k v_k + pad]; a node's box the exact min / max over its children that exist and
 *            are present; a node without a present child is absent itself (no ray passes it).
 * Stream     runs on the context's stream: a 12-byte memset and a handful of kernels in a linear chain (three for up to 65 536
 *            triangles).  Allocates nothing, does not synchronise, may be recorded under stream capture, may be called every frame.
 * stats      DEVICE pointer to 4 words, or NULL (as the rasteriser's): [0] present triangles, [1] absent triangles, [2] the bits of S
 *            (fp32), [3] 0; written on the stream.
 * sah_debug_rt_structure after a refit reports in header[3] the pad the device used (it waits for the stream to read it).
 *
 * SAH_ERR_INVALID_ARGUMENT: ctx or scene NULL; no sah_rt_build on this context yet; one of the three counts differs; a NULL array with
 * num_primitives > 0.  A structure of 0 triangles: SAH_OK, nothing is launched (stats, when given, are zeroed on the stream). */
int sah_rt_refit(sah_ctx* ctx, const sah_scene_geometry* scene, uint32_t* stats);

#ifdef __cplusplus
}
#endif

#endif /* SAH_RT_REFIT_H */
