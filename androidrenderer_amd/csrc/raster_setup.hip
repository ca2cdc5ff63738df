// Scene rasterisation as compute: the sun shadow cascades, the depth + G-buffer pass, the LPV's RSM and the
// motion vectors.  Stage 1 of 2 (this file): scan, vertex stage, clipping, set-up, binning; stage 2 is raster_tiles.hip.
//   reference: RenderCore/render/directional_light.cpp:286-327, RenderCore/render/phase/gbuffer_phase.cpp:27-97,
//              RenderCore/render/gi/light_propagation_volume.cpp:566-615 (RSM), RenderCore/render/material_pipelines.cpp:13-140,
//              RenderCore/shaders/materials/gltf_basic_pbr.slang:110-253, RenderCore/render/render_scene.cpp:196-222 (cull mode / front face)
// The reference uses the fixed-function rasteriser.  Here: a set-up kernel turns every (view, triangle) into window-space records
// (vertex stage, trivial accept or a queue for the clip kernel — Sutherland-Hodgman against the depth planes and a guard band, fan —
// then 24.8 snapping and culling), the records are binned to 64x64-pixel tiles (count, scan, fill), and one workgroup per tile
// resolves visibility in LDS (raster_tiles.hip).  Depth tests are order-independent by construction, so the images do not depend on
// the (nondeterministic) order of the bin lists.  The rasterisation rules — the part the API leaves to the implementation — are
// DESIGN.md §5d; arithmetic follows §3 (every fp32 operator individually rounded; half expressions rounded after every operator).
// k_bin lives here whole, although its fill form runs in stage 2: both forms share every line but the visit, and of this file they
// need nothing that raster_common.hpp does not already hold; stage 2 reaches it through launch_raster_fill_bins (launch.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "launch.hpp"
#include "numerics.hpp"
#include "prim_scan.hpp"
#include "raster_args.hpp"
#include "raster_common.hpp"

namespace sah {
namespace {

constexpr float kGuardBand = 16.0f;     // |x_c|, |y_c| <= kGuardBand * w_c survives clipping
constexpr float kCoordLimit = 0x1p24f + 4096.0f;  // snapped coordinates beyond this drop the triangle: edge functions stay below 2^52

struct ClipVertex {
    float c[4];
    float bary[3];
};

SAH_DEV float mat_row(const float* m, int r, float x, float y, float z, float w) { return ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w; }
SAH_DEV void mat_vec(const float* m, const float v[4], float out[4]) {
    for (int r = 0; r < 4; r++) out[r] = mat_row(m, r, v[0], v[1], v[2], v[3]);
}

SAH_DEV float plane_distance(const ClipVertex& v, int plane) {
    switch (plane) {
        case 0: return v.c[2];
        case 1: return v.c[3] - v.c[2];
        case 2: return kGuardBand * v.c[3] - v.c[0];
        case 3: return kGuardBand * v.c[3] + v.c[0];
        case 4: return kGuardBand * v.c[3] - v.c[1];
        default: return kGuardBand * v.c[3] + v.c[1];
    }
}
SAH_DEV ClipVertex lerp_vertex(const ClipVertex& in, const ClipVertex& out, float d_in, float d_out) {
    const float t = d_in / (d_in - d_out);
    ClipVertex r;
    for (int k = 0; k < 4; k++) r.c[k] = in.c[k] + (out.c[k] - in.c[k]) * t;
    for (int k = 0; k < 3; k++) r.bary[k] = in.bary[k] + (out.bary[k] - in.bary[k]) * t;
    return r;
}
// Sutherland-Hodgman in place (rare path: most triangles are inside every plane and skip it)
SAH_DEV int clip_polygon(ClipVertex* poly, ClipVertex* tmp, int n, int first_plane) {
    for (int plane = first_plane; plane < 6 && n >= 3; plane++) {
        int m = 0;
        for (int i = 0; i < n; i++) {
            const ClipVertex a = poly[i];
            const ClipVertex b = poly[i + 1 == n ? 0 : i + 1];
            const float da = plane_distance(a, plane), db = plane_distance(b, plane);
            const bool ia = da >= 0.0f, ib = db >= 0.0f;
            if (ia) tmp[m++] = a;
            if (ia != ib) tmp[m++] = ia ? lerp_vertex(a, b, da, db) : lerp_vertex(b, a, db, da);
        }
        n = m;
        for (int i = 0; i < n; i++) poly[i] = tmp[i];
    }
    return n < 3 ? 0 : n;
}

struct WindowVertex {
    int32_t X, Y;
    float z, inv_w;
    float bary[3];
    bool finite;
};
SAH_DEV bool is_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }
SAH_DEV WindowVertex to_window(const ClipVertex& v, float half_w, float half_h) {
    WindowVertex r;
    const float xd = v.c[0] / v.c[3], yd = v.c[1] / v.c[3];
    r.z = v.c[2] / v.c[3];
    r.inv_w = 1.0f / v.c[3];
    const float xf = xd * half_w + half_w, yf = yd * half_h + half_h;
    const float sx = xf * 256.0f, sy = yf * 256.0f;
    r.finite = is_finite(sx) && is_finite(sy) && is_finite(r.z) && is_finite(r.inv_w) && __builtin_fabsf(sx) <= kCoordLimit && __builtin_fabsf(sy) <= kCoordLimit;
    r.X = r.finite ? (int32_t)__builtin_rintf(sx) : 0;
    r.Y = r.finite ? (int32_t)__builtin_rintf(sy) : 0;
    for (int k = 0; k < 3; k++) r.bary[k] = v.bary[k];
    return r;
}

SAH_DEV int32_t first_px(int32_t lo) { const int32_t a = lo - 128; return a <= 0 ? 0 : (a + 255) >> 8; }
SAH_DEV int32_t last_px(int32_t hi, uint32_t size) {
    const int32_t a = hi - 128;
    if (a < 0) return -1;
    const int32_t p = a >> 8;
    return p < (int32_t)size - 1 ? p : (int32_t)size - 1;
}

// ---- K0: exclusive scan (single workgroup, chunked: prim_scan.hpp) -----------------------------------------------------------------
// mode 0: in[i] = primitives[i].index_count / 3; mode 1: in[i] = values[i]
__global__ __launch_bounds__(1024) void k_exclusive_scan(const sah_primitive* prims, const uint32_t* values, uint32_t n, uint32_t* out, uint32_t* total) {
    block_exclusive_scan<8>(n, [=](uint32_t i) { return prims ? prims[i].index_count / 3u : values[i]; }, out, total);
}

// the scan of the translucent pass: a primitive of another type contributes no triangle, so it owns no work item, no record and no
// sequence number (find_primitive never lands on a primitive without triangles)
__global__ __launch_bounds__(1024) void k_exclusive_scan_of_type(const sah_primitive* prims, uint32_t type, uint32_t n, uint32_t* out, uint32_t* total) {
    block_exclusive_scan<8>(n, [=](uint32_t i) { return prims[i].type == type ? prims[i].index_count / 3u : 0u; }, out, total);
}

// ---- K1: vertex stage, clipping, fan, snapping, culling -> records ----------------------------------------------------------------
// the half-precision varyings of one vertex (gltf_basic_pbr.slang:134-143): colour, normalize(model3x3 * normal), tangent
SAH_DEV void rotate_normalize(const float* m, const float v[3], uint16_t out[3]) {
    float r[3];
    for (int i = 0; i < 3; i++) r[i] = (m[i] * v[0] + m[4 + i] * v[1]) + m[8 + i] * v[2];
    const float inv = 1.0f / __builtin_sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    for (int i = 0; i < 3; i++) out[i] = f2h(r[i] * inv);
}
SAH_DEV void vertex_outputs(const sah_primitive& prim, const sah_vertex_data& vd, uint16_t out[12]) {
    for (int c = 0; c < 4; c++) out[c] = f2h((float)((vd.color >> (8 * c)) & 0xffu) / 255.0f);
    rotate_normalize(prim.model, vd.normal, out + 4);
    rotate_normalize(prim.model, vd.tangent, out + 7);
    out[10] = f2h(vd.tangent[3]);
    out[11] = 0;
}

constexpr uint32_t kAppend = 0xffffffffu;

struct SetupStats {
    uint32_t in = 0, culled = 0, dropped = 0, raster = 0;
};

// The set-up kernels are instantiated per attribute record, which is what tells the passes apart at this stage: ShadowAttr (shadow
// cascades: no near / far clipping, attributes for CUTOUT records only and only when the scene brought them), RasterAttr (G-buffer and
// RSM, told apart by a.rsm at run time) and MotionAttr (motion vectors: SOLID primitives only).  kWithMotion beside RasterAttr is the
// set-up of sah_gbuffer_motion_render: the G-buffer's, which also writes the MotionAttr of every record of a SOLID primitive.  Slot,
// sequence number and RasterRecord of such a record are the stand-alone motion pass's: both count every primitive in the running
// triangle number (k_setup skips a CUTOUT one only after `t` is fixed), both run clip_vertex / clip_polygon / to_window on the same
// inputs (a.rsm is 0 in both), and emit_triangle derives the record from those alone.  One difference remains: the G-buffer's range
// check reads the material, the motion pass's does not (sah_gbuffer_motion.h says what follows).
template <class Attr> constexpr bool kShadowSetup = std::is_same_v<Attr, ShadowAttr>;
template <class Attr> constexpr bool kMotionSetup = std::is_same_v<Attr, MotionAttr>;

// motion_vectors.vert.slang:27-31: the same model matrix serves both frames
SAH_DEV void write_motion_attr(const RasterArgs& a, const sah_primitive& prim, uint32_t tri, const WindowVertex& v0, const WindowVertex& v1, const WindowVertex& v2,
                               uint32_t r) {
    MotionAttr ma;
    ma.inv_w[0] = v0.inv_w; ma.inv_w[1] = v1.inv_w; ma.inv_w[2] = v2.inv_w;
    for (int k = 0; k < 3; k++) { ma.bary[0][k] = v0.bary[k]; ma.bary[1][k] = v1.bary[k]; ma.bary[2][k] = v2.bary[k]; }
    for (int k = 0; k < 3; k++) {
        const float* pos = a.positions + 3 * ((int64_t)prim.vertex_offset + a.indices[prim.first_index + 3 * tri + k]);
        const float local[4] = {pos[0], pos[1], pos[2], 1.0f};
        float world[4], vs[4], prev[4];
        mat_vec(prim.model, local, world);
        mat_vec(a.prev_view_matrix, world, vs);
        mat_vec(a.prev_clip_matrix, vs, prev);
        ma.prev[k][0] = prev[0]; ma.prev[k][1] = prev[1]; ma.prev[k][2] = prev[3];
    }
    a.motion_attrs[r] = ma;
}

// One window-space triangle of the fan: facing, bounding box, record.
template <class Attr, bool kWithMotion>
SAH_DEV void emit_triangle(const RasterArgs& a, SetupStats& st, uint32_t view, uint32_t p, const sah_primitive& prim, uint32_t tri, uint32_t seq,
                           const WindowVertex& v0, WindowVertex v1, WindowVertex v2, uint32_t slot) {
    if (!v0.finite || !v1.finite || !v2.finite) { st.dropped++; return; }
    const int64_t area = (int64_t)(v1.X - v0.X) * (v2.Y - v0.Y) - (int64_t)(v2.X - v0.X) * (v1.Y - v0.Y);
    if (area == 0 || (area < 0 && prim.type == SAH_PRIMITIVE_TYPE_SOLID)) { st.culled++; return; }
    if (area < 0) { const WindowVertex s = v1; v1 = v2; v2 = s; }
    const int32_t minx = min(v0.X, min(v1.X, v2.X)), maxx = max(v0.X, max(v1.X, v2.X));
    const int32_t miny = min(v0.Y, min(v1.Y, v2.Y)), maxy = max(v0.Y, max(v1.Y, v2.Y));
    const int32_t x0 = first_px(minx), x1 = last_px(maxx, a.width), y0 = first_px(miny), y1 = last_px(maxy, a.height);
    if (x0 > x1 || y0 > y1) { st.culled++; return; }
    st.raster++;
    // Unclipped triangles own the slot of their work item (no allocation: a single-address atomic per wave was the bottleneck of this
    // kernel); the fans of clipped ones are appended behind those.
    const uint32_t r = slot != kAppend ? slot : a.counters[C_TRIS] * a.num_views + wave_alloc(&a.counters[C_RECORDS], true);
    if (r >= a.record_capacity) return;  // the host sees the counts, grows the buffer and runs the pass again
    RasterRecord rec;
    rec.X[0] = v0.X; rec.X[1] = v1.X; rec.X[2] = v2.X;
    rec.Y[0] = v0.Y; rec.Y[1] = v1.Y; rec.Y[2] = v2.Y;
    rec.z[0] = v0.z; rec.z[1] = v1.z; rec.z[2] = v2.z;
    rec.view = view;
    rec.x0 = (uint16_t)x0; rec.x1 = (uint16_t)x1; rec.y0 = (uint16_t)y0; rec.y1 = (uint16_t)y1;
    rec.seq = seq;
    // masked geometry is alpha-tested in every pass (shadow_masked_pso / rsm_masked_pso / gbuffer_masked_pso, material_pipelines.cpp:47-140)
    rec.cutout = prim.type == SAH_PRIMITIVE_TYPE_CUTOUT && (!kShadowSetup<Attr> || a.shadow_attrs != nullptr);
    a.records[r] = rec;
    if (kShadowSetup<Attr> && prim.type == SAH_PRIMITIVE_TYPE_CUTOUT) {
        if (a.shadow_attrs) {
            ShadowAttr sa;
            sa.inv_w[0] = v0.inv_w; sa.inv_w[1] = v1.inv_w; sa.inv_w[2] = v2.inv_w;
            for (int k = 0; k < 3; k++) { sa.bary[0][k] = v0.bary[k]; sa.bary[1][k] = v1.bary[k]; sa.bary[2][k] = v2.bary[k]; }
            for (int k = 0; k < 3; k++) {
                const sah_vertex_data& vd = a.vertex_data[(int64_t)prim.vertex_offset + a.indices[prim.first_index + 3 * tri + k]];
                sa.alpha[k] = f2h((float)((vd.color >> 24) & 0xffu) / 255.0f);
            }
            sa.pad = 0;
            sa.material = prim.material;
            sa.pad2 = 0;
            for (int k = 0; k < 3; k++) {
                const sah_vertex_data& vd = a.vertex_data[(int64_t)prim.vertex_offset + a.indices[prim.first_index + 3 * tri + k]];
                sa.uv[k][0] = vd.texcoord[0];
                sa.uv[k][1] = vd.texcoord[1];
            }
            sa.pad3[0] = sa.pad3[1] = 0;
            a.shadow_attrs[r] = sa;
        } else {
            atomicAdd(&a.counters[C_CUTOUT_NO_ATTR], 1u);  // the host turns this into SAH_ERR_INVALID_ARGUMENT (api_raster.cpp)
        }
    }
    if (kMotionSetup<Attr> || (kWithMotion && prim.type == SAH_PRIMITIVE_TYPE_SOLID)) write_motion_attr(a, prim, tri, v0, v1, v2, r);
    if (std::is_same_v<Attr, RasterAttr>) {
        RasterAttr at;
        at.inv_w[0] = v0.inv_w; at.inv_w[1] = v1.inv_w; at.inv_w[2] = v2.inv_w;
        for (int k = 0; k < 3; k++) { at.bary[0][k] = v0.bary[k]; at.bary[1][k] = v1.bary[k]; at.bary[2][k] = v2.bary[k]; }
        at.primitive = p;
        at.material = prim.material;
        at.seq = seq;
        at.cutout = prim.type == SAH_PRIMITIVE_TYPE_CUTOUT;
        for (int k = 0; k < 3; k++) {
            const sah_vertex_data& vd = a.vertex_data[(int64_t)prim.vertex_offset + a.indices[prim.first_index + 3 * tri + k]];
            vertex_outputs(prim, vd, at.vout[k]);
            at.uv[k][0] = vd.texcoord[0];
            at.uv[k][1] = vd.texcoord[1];
        }
        a.attrs[r] = at;
    }
}

// vertex stage of corner k of input triangle `tri` (gltf_basic_pbr.slang:126-133)
template <class Attr>
SAH_DEV ClipVertex clip_vertex(const RasterArgs& a, const sah_primitive& prim, uint32_t view, uint32_t tri, int k) {
    const uint32_t idx = a.indices[prim.first_index + 3 * tri + k];
    const float* pos = a.positions + 3 * ((int64_t)prim.vertex_offset + idx);
    const float local[4] = {pos[0], pos[1], pos[2], 1.0f};
    float world[4], clip[4];
    mat_vec(prim.model, local, world);
    if (!kShadowSetup<Attr> && !a.rsm) {
        float vs[4];
        mat_vec(a.view_matrix, world, vs);
        mat_vec(a.clip_matrix[0], vs, clip);
    } else {  // shadow cascades and RSM layers: one world -> clip matrix per view
        mat_vec(a.clip_matrix[view], world, clip);
    }
    ClipVertex c;
    for (int j = 0; j < 4; j++) c.c[j] = clip[j];
    for (int j = 0; j < 3; j++) c.bary[j] = j == k ? 1.0f : 0.0f;
    return c;
}

// Rare path: the triangle crosses a clipping plane.  k_setup queues it and this kernel, launched right after, clips and fans it, so
// that the polygon arrays (scratch memory) and their registers burden only the triangles that need them.
template <class Attr, bool kWithMotion = false>
__global__ __launch_bounds__(64) void k_setup_clipped(const RasterArgs a) {
    // the polygons live in LDS, 12 vertices per lane and buffer: dynamically indexed private arrays would sit in scratch memory,
    // and the clipping loop is one long chain of dependent accesses to them
    __shared__ ClipVertex s_poly[64 * 12], s_tmp[64 * 12];
    const uint32_t queued = min(a.counters[C_CLIPPED], a.clip_capacity);
    SetupStats st;
    ClipVertex* poly = s_poly + threadIdx.x * 12;
    for (uint32_t q = blockIdx.x * 64 + threadIdx.x; q < queued; q += gridDim.x * 64) {
        const uint32_t view = a.clip_queue[q].x, t = a.clip_queue[q].y;
        const uint32_t p = find_primitive(a.tri_base, a.num_primitives, t);
        const sah_primitive& prim = a.primitives[p];
        const uint32_t tri = t - a.tri_base[p];
        for (int k = 0; k < 3; k++) poly[k] = clip_vertex<Attr>(a, prim, view, tri, k);
        const int n = clip_polygon(poly, s_tmp + threadIdx.x * 12, 3, kShadowSetup<Attr> ? 2 : 0);
        if (n == 0) { st.culled++; continue; }
        const WindowVertex v0 = to_window(poly[0], a.half_w, a.half_h);
        WindowVertex prev = to_window(poly[1], a.half_w, a.half_h);
        for (int i = 1; i + 1 < n; i++) {
            const WindowVertex next = to_window(poly[i + 1], a.half_w, a.half_h);
            emit_triangle<Attr, kWithMotion>(a, st, view, p, prim, tri, t * 8u + (uint32_t)(i - 1), v0, prev, next, kAppend);
            prev = next;
        }
    }
    __shared__ uint32_t s_acc[4];
    const uint32_t local[4] = {0u, st.culled, st.dropped, st.raster};
    block_flush<4>(&a.counters[C_STATS], local, s_acc);
}

template <class Attr, bool kWithMotion = false>
__global__ __launch_bounds__(256) void k_setup(const RasterArgs a) {
    const uint32_t total = a.counters[C_TRIS];
    const uint64_t work = (uint64_t)total * a.num_views;
    SetupStats st;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < work; w += (uint64_t)gridDim.x * 256) {
        const uint32_t view = (uint32_t)(w / total), t = (uint32_t)(w % total);
        const uint32_t p = find_primitive(a.tri_base, a.num_primitives, t);
        const sah_primitive& prim = a.primitives[p];
        const uint32_t tri = t - a.tri_base[p];
        st.in++;
        if (w < a.record_capacity) mark_empty(a.records[w]);  // overwritten below if the triangle survives unclipped
        if (kMotionSetup<Attr> && prim.type != SAH_PRIMITIVE_TYPE_SOLID) { st.culled++; continue; }  // scene.draw_opaque: nothing else is drawn
        // a draw that points outside the index / vertex / material arrays is dropped, never dereferenced
        // (the material is read for every record of the G-buffer and RSM passes, for the CUTOUT records of a shadow pass that has
        //  attributes, never by the motion-vectors pass)
        constexpr bool kMaterialOfEveryRecord = std::is_same_v<Attr, RasterAttr>;
        bool in_range = (uint64_t)prim.first_index + 3ull * tri + 3ull <= a.num_indices &&
                        (kMotionSetup<Attr> || !(kMaterialOfEveryRecord || (a.shadow_attrs && prim.type == SAH_PRIMITIVE_TYPE_CUTOUT)) || prim.material < a.num_materials);
        for (int k = 0; k < 3 && in_range; k++) {
            const int64_t v = (int64_t)prim.vertex_offset + a.indices[prim.first_index + 3 * tri + k];
            in_range = v >= 0 && v < (int64_t)a.num_vertices;
        }
        if (!in_range) { st.dropped++; continue; }
        const ClipVertex c0 = clip_vertex<Attr>(a, prim, view, tri, 0), c1 = clip_vertex<Attr>(a, prim, view, tri, 1),
                         c2 = clip_vertex<Attr>(a, prim, view, tri, 2);
        bool finite = true, inside = true;
        for (int j = 0; j < 4; j++) finite = finite && is_finite(c0.c[j]) && is_finite(c1.c[j]) && is_finite(c2.c[j]);
        for (int plane = kShadowSetup<Attr> ? 2 : 0; plane < 6; plane++)
            inside = inside && plane_distance(c0, plane) >= 0.0f && plane_distance(c1, plane) >= 0.0f && plane_distance(c2, plane) >= 0.0f;
        if (!finite) { st.dropped++; continue; }
        if (inside) {
            emit_triangle<Attr, kWithMotion>(a, st, view, p, prim, tri, t * 8u, to_window(c0, a.half_w, a.half_h), to_window(c1, a.half_w, a.half_h),
                                   to_window(c2, a.half_w, a.half_h), w < a.record_capacity ? (uint32_t)w : a.record_capacity);
        } else {
            const uint32_t q = wave_alloc(&a.counters[C_CLIPPED], true);
            if (q < a.clip_capacity) a.clip_queue[q] = make_uint2(view, t);  // overflow: the host sees the count and runs the pass again
        }
    }
    __shared__ uint32_t s_acc[4];
    const uint32_t local[4] = {st.in, st.culled, st.dropped, st.raster};
    block_flush<4>(&a.counters[C_STATS], local, s_acc);
}

// ---- K2 / K4: binning -------------------------------------------------------------------------------------------------------------
// One wave per 64 records.  A record that touches up to 4 tiles is binned by its own lane; wider ones are taken one at a time by the
// whole wave (ballot + readlane), lanes striding over the tiles of the bounding box.
template <bool FILL>
__global__ __launch_bounds__(256) void k_bin(const RasterArgs a) {
    const uint32_t nrec = record_count(a);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * 4u;
    uint32_t st_pairs = 0;
    // records per wave: 64 when there are plenty, fewer when the scene is a handful of screen-filling triangles (each of which is
    // a long loop over tiles that should not queue up behind 63 others in one wave)
    const uint32_t per_wave = min(64u, max(1u, (nrec + waves - 1) / waves));
    for (uint32_t base = (blockIdx.x * 4u + (threadIdx.x >> 6)) * per_wave; base < nrec; base += waves * per_wave) {
        const uint32_t r = base + lane;
        uint32_t tx0 = 1, tx1 = 0, ty0 = 1, ty1 = 0, view = 0;
        bool live = false;
        if (lane < per_wave && r < nrec) {
            const RasterRecord& rec = a.records[r];
            live = !is_empty(rec);
            if (live) { tx0 = rec.x0 / kTile; tx1 = rec.x1 / kTile; ty0 = rec.y0 / kTile; ty1 = rec.y1 / kTile; view = rec.view; }
        }
        const uint32_t ntiles = live ? (tx1 - tx0 + 1) * (ty1 - ty0 + 1) : 0u;
        auto visit = [&](uint32_t tile, uint32_t rec_index) {
            if (FILL) {
                const uint32_t pos = atomicAdd(&a.tile_cursor[tile], 1u);
                const uint32_t at = a.tile_offset[tile] + pos;
                if (at < a.pairs_capacity) a.pairs[at] = rec_index;  // a short list is noticed by the host, which grows it and repeats the pass
            } else {
                atomicAdd(&a.tile_count[tile], 1u);
                st_pairs++;
            }
        };
        // single-tile records (most of a dense mesh): neighbouring triangles land in the same few tiles, so the lanes that share a tile
        // share one atomic — per-address atomic throughput is what bounds this kernel
        uint64_t single = __ballot(ntiles == 1);
        const uint32_t my_tile = (view * a.tiles_y + ty0) * a.tiles_x + tx0;
        while (single) {
            const int leader = __builtin_ctzll(single);
            const uint32_t tile = __shfl(my_tile, leader, 64);
            const uint64_t same = __ballot(ntiles == 1 && my_tile == tile) & single;
            single &= ~same;
            const uint32_t n = (uint32_t)__builtin_popcountll(same);
            const bool mine = (same >> lane) & 1ull;
            if (FILL) {
                uint32_t first = 0;
                if ((int)lane == leader) first = atomicAdd(&a.tile_cursor[tile], n);
                first = __shfl(first, leader, 64);
                const uint32_t at = a.tile_offset[tile] + first + (uint32_t)__builtin_popcountll(same & ((1ull << lane) - 1ull));
                if (mine && at < a.pairs_capacity) a.pairs[at] = r;
            } else {
                if ((int)lane == leader) atomicAdd(&a.tile_count[tile], n);
                st_pairs += mine ? 1u : 0u;
            }
        }
        if (ntiles > 1 && ntiles <= 4)
            for (uint32_t ty = ty0; ty <= ty1; ty++)
                for (uint32_t tx = tx0; tx <= tx1; tx++) visit((view * a.tiles_y + ty) * a.tiles_x + tx, r);
        uint64_t wide = __ballot(ntiles > 4);
        while (wide) {
            const int src = __builtin_ctzll(wide);
            wide &= wide - 1;
            const uint32_t bx0 = __shfl(tx0, src, 64), bx1 = __shfl(tx1, src, 64), by0 = __shfl(ty0, src, 64), by1 = __shfl(ty1, src, 64);
            const uint32_t bview = __shfl(view, src, 64), bw = bx1 - bx0 + 1, count = bw * (by1 - by0 + 1);
            // a tile of the bounding box that lies wholly outside one edge gets no entry (about half the tiles of a large triangle);
            // both binning passes run the same exact test, so count and fill agree
            const RasterRecord& wrec = a.records[base + (uint32_t)src];
            for (uint32_t i = lane; i < count; i += 64) {
                const uint32_t tx = bx0 + i % bw, ty = by0 + i / bw;
                if (count < 16 || !tile_outside(wrec, (int32_t)(tx * kTile), (int32_t)(ty * kTile))) visit((bview * a.tiles_y + ty) * a.tiles_x + tx, base + (uint32_t)src);
            }
        }
    }
    __shared__ uint32_t s_acc[1];
    const uint32_t local[1] = {FILL ? 0u : st_pairs};
    block_flush<1>(&a.counters[C_STATS + 4], local, s_acc);
}

// one thread per texture slot and per material: anything the fragment stages could not sample safely is counted, and the host fails the call
__global__ __launch_bounds__(256) void k_check_textures(const RasterArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < a.num_textures) {
        const sah_texture& T = a.textures[i];
        bad = T.num_mips < 1 || T.num_mips > SAH_MAX_TEXTURE_MIPS || T.sampler.mag_filter > 1 || T.sampler.min_filter > 1 || T.sampler.mipmap_mode > 1 ||
              T.sampler.address_u > 2 || T.sampler.address_v > 2 || T.sampler.max_anisotropy > 16.0f;
        for (uint32_t l = 0; !bad && l < T.num_mips; l++) {
            const sah_plane& p = T.mips[l];
            bad = !p.ptr || p.width == 0 || p.height == 0 || p.width > 16384 || p.height > 16384 || p.format != T.mips[0].format ||
                  (p.format != SAH_FORMAT_R8G8B8A8_UNORM && p.format != SAH_FORMAT_R8G8B8A8_SRGB) || p.row_pitch_bytes < p.width * 4u;
        }
    } else if (i - a.num_textures < a.num_materials) {
        const sah_material_textures mt = a.material_textures[i - a.num_textures];
        const uint32_t idx[4] = {mt.base_color, mt.normal, mt.data, mt.emission};
        for (int k = 0; k < 4; k++) bad = bad || (idx[k] != SAH_TEXTURE_NONE && idx[k] >= a.num_textures);
    }
    if (bad) atomicAdd(&a.counters[C_BAD_TEXTURE], 1u);
}

template <class Attr, bool kWithMotion = false>
void launch_setup_kernels(const RasterArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((k_setup<Attr, kWithMotion>), dim3(1024), dim3(256), 0, st, a);
    hipLaunchKernelGGL((k_setup_clipped<Attr, kWithMotion>), dim3(256), dim3(64), 0, st, a);
}

}  // namespace

// Stage 1: scan the draws, set up the records, count the bins, scan the bins.  The caller then reads `counters` back.
hipError_t launch_raster_setup(const RasterArgs& a, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.counters, 0, C_WORDS * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const uint32_t ntiles = a.tiles_x * a.tiles_y * a.num_views;
    e = hipMemsetAsync(a.tile_count, 0, (size_t)ntiles * 2 * sizeof(uint32_t), st);  // tile_count and tile_cursor are adjacent
    if (e != hipSuccess) return e;
    if (a.num_primitives == 0) return hipSuccess;
    if (a.textures) hipLaunchKernelGGL(k_check_textures, dim3((a.num_textures + a.num_materials + 255u) / 256u), dim3(256), 0, st, a);
    if (a.pass == RasterPass::Translucent)
        hipLaunchKernelGGL(k_exclusive_scan_of_type, dim3(1), dim3(1024), 0, st, a.primitives, (uint32_t)SAH_PRIMITIVE_TYPE_TRANSLUCENT, a.num_primitives, a.tri_base,
                           &a.counters[C_TRIS]);
    else
        hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, st, a.primitives, (const uint32_t*)nullptr, a.num_primitives, a.tri_base, &a.counters[C_TRIS]);
    switch (a.pass) {
        case RasterPass::Shadow: launch_setup_kernels<ShadowAttr>(a, st); break;
        case RasterPass::GBuffer:
        case RasterPass::Rsm:
        case RasterPass::Translucent: launch_setup_kernels<RasterAttr>(a, st); break;
        case RasterPass::Motion: launch_setup_kernels<MotionAttr>(a, st); break;
        case RasterPass::GBufferMotion: launch_setup_kernels<RasterAttr, true>(a, st); break;
    }
    hipLaunchKernelGGL(k_bin<false>, dim3(1024), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, st, (const sah_primitive*)nullptr, (const uint32_t*)a.tile_count, ntiles, a.tile_offset, &a.counters[C_PAIRS]);
    return hipGetLastError();
}

// First kernel of stage 2 (launch_raster_tiles): the bin lists, now that their offsets are known.
void launch_raster_fill_bins(const RasterArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_bin<true>, dim3(1024), dim3(256), 0, st, a); }

}  // namespace sah
