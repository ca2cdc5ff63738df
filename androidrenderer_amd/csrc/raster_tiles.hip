// Scene rasterisation as compute, stage 2 of 2 (stage 1 and the overview: raster_setup.hip): one workgroup per 64x64 tile, or per part
// of a long bin list, resolves visibility in LDS — sweeping 8x8 pixel blocks with exact fp64 edge functions (raster_common.hpp) — then
// shades and writes its tile once, coalesced.  ONE tile kernel serves the four passes: what a pass does with a covered pixel, what
// it keeps per pixel and how it turns that into images is its *target* (ShadowTarget, GBufferTarget — RSM included —, MotionTarget);
// the walk over the bin list, the split-list merge and the look-up from a sequence number to its record are written once.  The translucent
// pass (sah_translucent.h) has a tile kernel of its own at the end of the file, which keeps every fragment of a pixel where the targets
// keep one: it reuses the walk, the look-up and the G-buffer's fragment stage as they are.
//   reference for the fragment stages: RenderCore/shaders/materials/gltf_basic_pbr.slang:169-253, RenderCore/render/material_pipelines.cpp:13-140,
//              RenderCore/render/phase/motion_vectors_phase.cpp:55-103
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "launch.hpp"
#include "lighting_common.hpp"
#include "numerics.hpp"
#include "raster_args.hpp"
#include "raster_common.hpp"
#include "texture_sample.hpp"

namespace sah {
namespace {

#ifndef SAH_RASTER_SMALL_AREA
#define SAH_RASTER_SMALL_AREA 64  // 4 / 16 / 64 measured: 64 is best for dense meshes (-8 %), neutral elsewhere
#endif
#ifndef SAH_RASTER_MEDIUM_AREA
#define SAH_RASTER_MEDIUM_AREA 1024  // 256 / 1024 / 4096 measured
#endif
constexpr uint32_t kSmallArea = SAH_RASTER_SMALL_AREA;    // (bbox ∩ tile) pixel count up to which one lane walks a triangle alone
constexpr uint32_t kMediumArea = SAH_RASTER_MEDIUM_AREA;  // ... up to which one wave does; above, the whole workgroup

constexpr uint32_t kTileThreads = 256;   // 1024 (16 waves per tile, to shorten the densest tiles) measured 1.1x - 2.5x slower
constexpr uint32_t kSplit = kRasterSplit;  // bin lists longer than this are cut into parts of this many entries, one workgroup each
constexpr uint32_t kBigSlots = 64;       // workgroup-cooperative records per round of list entries; the rest fall back to their wave

// ---- fragment stages ------------------------------------------------------------------------------------------------------------------
// perspective-correct barycentrics in the INPUT triangle, from the screen-space ones of the record
SAH_DEV void input_barycentrics(const float inv_w[3], const float (&bary)[3][3], const float b[3], float lambda[3]) {
    const float q0 = b[0] * inv_w[0], q1 = b[1] * inv_w[1], q2 = b[2] * inv_w[2];
    const float s = (q0 + q1) + q2;
    const float l0 = q0 / s, l1 = q1 / s, l2 = q2 / s;
    for (int k = 0; k < 3; k++) lambda[k] = (l0 * bary[0][k] + l1 * bary[1][k]) + l2 * bary[2][k];
}
// varying `c` of the three vertices, interpolated in fp32 and rounded to half
SAH_DEV Hn interp_h(const RasterAttr& at, const float lambda[3], int c) {
    return Hn((lambda[0] * h2f(at.vout[0][c]) + lambda[1] * h2f(at.vout[1][c])) + lambda[2] * h2f(at.vout[2][c]));
}

SAH_DEV uint32_t unorm8_of(float c) {  // floor(c * 255 + 0.5) in fp32, clamped, NaN -> 0
    if (!(c > 0.0f)) return 0u;
    if (c >= 1.0f) return 255u;
    return (uint32_t)(c * 255.0f + 0.5f);
}

// perspective-correct barycentrics of pixel (px, py) in the input triangle — also for a pixel the triangle does not cover (the other
// pixels of a fragment's quad)
SAH_DEV void lambda_at(const EdgeSetup& e, const float inv_w[3], const float (&bary)[3][3], int32_t px, int32_t py, float lambda[3]) {
    double v[3];
    float b[3];
    cover(e, px, py, v);
    barycentrics(e, v, b);
    input_barycentrics(inv_w, bary, b, lambda);
}
struct TexCoord {
    float t[2], ddx[2], ddy[2];
};
// the texcoord varying at the fragment and its fine derivatives over the 2x2 quad at even window coordinates
SAH_DEV TexCoord texcoord_of(const EdgeSetup& e, const float inv_w[3], const float (&bary)[3][3], const float (&uv)[3][2], int32_t px, int32_t py,
                             const float lambda[3]) {
    float lx[3], ly[3];
    lambda_at(e, inv_w, bary, px ^ 1, py, lx);
    lambda_at(e, inv_w, bary, px, py ^ 1, ly);
    TexCoord r;
    for (int c = 0; c < 2; c++) {
        const float t = (lambda[0] * uv[0][c] + lambda[1] * uv[1][c]) + lambda[2] * uv[2][c];
        const float tx = (lx[0] * uv[0][c] + lx[1] * uv[1][c]) + lx[2] * uv[2][c];
        const float ty = (ly[0] * uv[0][c] + ly[1] * uv[1][c]) + ly[2] * uv[2][c];
        r.t[c] = t;
        r.ddx[c] = (px & 1) ? t - tx : tx - t;
        r.ddy[c] = (py & 1) ? t - ty : ty - t;
    }
    return r;
}
SAH_DEV sah_material_textures textures_of(const RasterArgs& a, uint32_t material) {
    if (!a.material_textures) return {SAH_TEXTURE_NONE, SAH_TEXTURE_NONE, SAH_TEXTURE_NONE, SAH_TEXTURE_NONE};
    return a.material_textures[min(material, a.num_materials - 1u)];
}
SAH_DEV bool any_texture(const RasterArgs& a, const sah_material_textures& mt) {
    return mt.base_color < a.num_textures || mt.normal < a.num_textures || mt.data < a.num_textures || mt.emission < a.num_textures;
}
// (half4) of one material slot: the sampled texture, or the material's constant texel (an index beyond the table — reported through
// C_BAD_TEXTURE by k_check_textures — is never dereferenced)
SAH_DEV void material_texel(const RasterArgs& a, uint32_t index, const float (&constant)[4], const TexCoord& tc, Hn out[4]) {
    if (index >= a.num_textures || a.counters[C_BAD_TEXTURE] != 0u) {  // (a bad table fails the call: nothing of it is dereferenced)
        for (int c = 0; c < 4; c++) out[c] = Hn(constant[c]);
        return;
    }
    float texel[4];
    sample_texture(a.luts, a.textures[index], tc.t, tc.ddx, tc.ddy, a.shader_mip_bias, texel);
    for (int c = 0; c < 4; c++) out[c] = Hn(texel[c]);
}

// fragment stage of one triangle at one pixel (gltf_basic_pbr.slang:169-253, SAH_MAIN_VIEW, constant textures): what it writes to the four
// colour targets, in their formats, goes to sink(colour, normals, data, emission)
template <bool TEX, class Sink>
SAH_DEV void fragment_stage(const RasterArgs& a, const EdgeSetup& e, const RasterAttr& at, const sah_material& m, const sah_material_textures& mt, int32_t px,
                            int32_t py, Sink&& sink) {
    double v[3];
    float b[3], lambda[3];
    cover(e, px, py, v);
    barycentrics(e, v, b);
    input_barycentrics(at.inv_w, at.bary, b, lambda);
    Hn base_texel[4], normal_texel[4], data_texel[4], emission_texel[4];
    if (TEX) {
        TexCoord tc{};
        if (any_texture(a, mt)) tc = texcoord_of(e, at.inv_w, at.bary, at.uv, px, py, lambda);
        material_texel(a, mt.base_color, m.base_color_texel, tc, base_texel);
        material_texel(a, mt.normal, m.normal_texel, tc, normal_texel);
        material_texel(a, mt.data, m.data_texel, tc, data_texel);
        material_texel(a, mt.emission, m.emission_texel, tc, emission_texel);
    } else {
        for (int c = 0; c < 4; c++) {
            base_texel[c] = Hn(m.base_color_texel[c]);
            normal_texel[c] = Hn(m.normal_texel[c]);
            data_texel[c] = Hn(m.data_texel[c]);
            emission_texel[c] = Hn(m.emission_texel[c]);
        }
    }
    Hn col[4], N[3], T[4];
    for (int c = 0; c < 4; c++) col[c] = interp_h(at, lambda, c);
    for (int c = 0; c < 3; c++) N[c] = interp_h(at, lambda, 4 + c);
    for (int c = 0; c < 4; c++) T[c] = interp_h(at, lambda, 7 + c);
    Hn tinted[4];
    for (int c = 0; c < 4; c++) tinted[c] = base_texel[c] * col[c] * Hn(m.base_color_tint[c]);
    // bitangent = cross(normal, tangent.xyz) * tangent.w; normal = normal_sample * TBN (:197-207)
    const Hn B[3] = {(N[1] * T[2] - N[2] * T[1]) * T[3], (N[2] * T[0] - N[0] * T[2]) * T[3], (N[0] * T[1] - N[1] * T[0]) * T[3]};
    Hn ns[3], n_out[3];
    for (int c = 0; c < 3; c++) ns[c] = normal_texel[c] * Hn::lit(2.0f) - Hn::lit(1.0f);
    for (int c = 0; c < 3; c++) n_out[c] = ns[0] * T[c] + ns[1] * B[c] + ns[2] * N[c];
    const float factor[4] = {0.0f, m.roughness_factor, m.metalness_factor, 0.0f};
    uint32_t color_bits = 0, data_bits = 0, emission_bits = 0;
    for (int c = 0; c < 4; c++) {
        const Hn d = data_texel[c] * Hn(factor[c]);
        const Hn em = emission_texel[c] * Hn(m.emission_factor[c]);
        data_bits |= unorm8_of(tof(d)) << (8 * c);
        emission_bits |= (c < 3 ? (uint32_t)a.half_to_srgb8[__builtin_bit_cast(uint16_t, em.v)] : unorm8_of(tof(em))) << (8 * c);
        color_bits |= (c < 3 ? (uint32_t)a.half_to_srgb8[__builtin_bit_cast(uint16_t, tinted[c].v)] : unorm8_of(tof(tinted[c]))) << (8 * c);
    }
    uint2 nbits;
    nbits.x = (uint32_t)__builtin_bit_cast(uint16_t, n_out[0].v) | ((uint32_t)__builtin_bit_cast(uint16_t, n_out[1].v) << 16);
    nbits.y = (uint32_t)__builtin_bit_cast(uint16_t, n_out[2].v);
    sink(color_bits, nbits, data_bits, emission_bits);
}
// ... of the winning triangle of the G-buffer pass, stored with its depth
template <bool TEX>
SAH_DEV void shade_and_store(const RasterArgs& a, const EdgeSetup& e, const RasterAttr& at, const sah_material& m, const sah_material_textures& mt, int32_t px,
                             int32_t py, float z) {
    fragment_stage<TEX>(a, e, at, m, mt, px, py, [&](uint32_t color_bits, uint2 nbits, uint32_t data_bits, uint32_t emission_bits) {
        *(uint32_t*)(a.out_color.ptr + (size_t)py * a.out_color.pitch + (size_t)px * 4) = color_bits;
        *(uint2*)(a.out_normals.ptr + (size_t)py * a.out_normals.pitch + (size_t)px * 8) = nbits;
        *(uint32_t*)(a.out_data.ptr + (size_t)py * a.out_data.pitch + (size_t)px * 4) = data_bits;
        *(uint32_t*)(a.out_emission.ptr + (size_t)py * a.out_emission.pitch + (size_t)px * 4) = emission_bits;
        *(float*)(a.out_depth.ptr + (size_t)py * a.out_depth.pitch + (size_t)px * 4) = z;
    });
}

// RSM fragment stage of the winning triangle (gltf_basic_pbr.slang:169-253, SAH_RSM): flux = Fd(surface, -sun direction, normal) with
// the metalness / roughness this variant leaves at 0, normal * 0.5 + 0.5; the D16 code goes to the depth layer
template <bool TEX>
SAH_DEV void shade_rsm_and_store(const RasterArgs& a, const EdgeSetup& e, const RasterAttr& at, const sah_material& m, const sah_material_textures& mt, uint32_t layer,
                                 int32_t px, int32_t py, uint32_t depth_code) {
    double v[3];
    float b[3], lambda[3];
    cover(e, px, py, v);
    barycentrics(e, v, b);
    input_barycentrics(at.inv_w, at.bary, b, lambda);
    Hn base_texel[4];
    if (TEX) {
        TexCoord tc{};
        if (mt.base_color < a.num_textures) tc = texcoord_of(e, at.inv_w, at.bary, at.uv, px, py, lambda);
        material_texel(a, mt.base_color, m.base_color_texel, tc, base_texel);
    } else {
        for (int c = 0; c < 4; c++) base_texel[c] = Hn(m.base_color_texel[c]);
    }
    Hn tinted[3], N[3];
    for (int c = 0; c < 3; c++) tinted[c] = base_texel[c] * interp_h(at, lambda, c) * Hn(m.base_color_tint[c]);
    for (int c = 0; c < 3; c++) N[c] = interp_h(at, lambda, 4 + c);
    Surface<Hn> s;
    s.base_color = {tinted[0], tinted[1], tinted[2]};
    s.normal = {N[0], N[1], N[2]};
    s.metalness = Hn::lit(0.0f);
    s.roughness = Hn::lit(0.0f);
    const V3<Hn> l = {-Hn(a.sun_direction[0]), -Hn(a.sun_direction[1]), -Hn(a.sun_direction[2])};
    const V3<Hn> flux = Fd(s, l, s.normal);
    const uint32_t flux_bits = (uint32_t)a.half_to_srgb8[__builtin_bit_cast(uint16_t, flux.x.v)] | ((uint32_t)a.half_to_srgb8[__builtin_bit_cast(uint16_t, flux.y.v)] << 8) |
                               ((uint32_t)a.half_to_srgb8[__builtin_bit_cast(uint16_t, flux.z.v)] << 16) | 0xff000000u;
    uint32_t normal_bits = 0xff000000u;
    for (int c = 0; c < 3; c++) normal_bits |= unorm8_of(tof(N[c] * Hn::lit(0.5f) + Hn::lit(0.5f))) << (8 * c);
    *(uint32_t*)(a.rsm_flux.ptr + (size_t)layer * a.rsm_flux.slice_pitch + (size_t)py * a.rsm_flux.row_pitch + (size_t)px * 4) = flux_bits;
    *(uint32_t*)(a.rsm_normals.ptr + (size_t)layer * a.rsm_normals.slice_pitch + (size_t)py * a.rsm_normals.row_pitch + (size_t)px * 4) = normal_bits;
    *(uint16_t*)(a.rsm_depth.ptr + (size_t)layer * a.rsm_depth.slice_pitch + (size_t)py * a.rsm_depth.row_pitch + (size_t)px * 2) = (uint16_t)depth_code;
}

// ---- motion vectors (sah_motion_vectors.h): MotionVectorsPhase::render, motion_vectors_phase.cpp:55-103 ----------------------------
// fragment stage of the winning triangle (motion_vectors_opaque.frag.slang:18-24); SV_Position.xy is the pixel centre
SAH_DEV uint32_t motion_vector_of(const RasterArgs& a, const EdgeSetup& e, const MotionAttr& ma, int32_t px, int32_t py) {
    float lambda[3], v[3];
    lambda_at(e, ma.inv_w, ma.bary, px, py, lambda);
    for (int c = 0; c < 3; c++) v[c] = (lambda[0] * ma.prev[0][c] + lambda[1] * ma.prev[1][c]) + lambda[2] * ma.prev[2][c];
    const float centre[2] = {(float)px + 0.5f, (float)py + 0.5f};
    uint32_t bits = 0;
    for (int c = 0; c < 2; c++) {
        const float ndc = v[c] / v[2];
        const float uv = ndc * 0.5f + 0.5f;
        const float mv = uv * a.render_resolution[c] - centre[c];
        bits |= (uint32_t)f2h(mv) << (16 * c);
    }
    return bits;
}

// ---- the work of one workgroup ----------------------------------------------------------------------------------------------------------
struct TileWork {
    uint32_t tile, part, parts;  // the tile, which part of its bin list, of how many (1: the list is walked whole)
    uint32_t begin, count;       // the part's entries: pairs[begin .. begin + count)
    uint32_t slot;               // merge buffer and ticket of a split tile (parts > 1)
    int32_t tile_x, tile_y;      // the tile's first pixel
    uint32_t view;
};
// Workgroups 0 .. ntiles-1 own a tile (and part 0 of its list); the rest take the further parts of the lists that k_split cut into
// pieces of kSplit entries: the densest tiles of a scene would otherwise set the duration of the whole kernel.  false: nothing to do.
SAH_DEV bool tile_work(const RasterArgs& a, TileWork& w) {
    const uint32_t ntiles = a.tiles_x * a.tiles_y * a.num_views;
    w.tile = blockIdx.x;
    w.part = 0;
    if (blockIdx.x >= ntiles) {
        const uint32_t k = blockIdx.x - ntiles;
        if (k >= min(a.counters[C_EXTRA], a.extra_capacity)) return false;
        w.tile = a.extra_parts[k].x;
        w.part = a.extra_parts[k].y;
        if (w.tile >= ntiles) return false;  // never for a pass whose buffers were large enough (a too-small pass is repeated by the host)
    }
    w.tile_x = (int32_t)(w.tile % a.tiles_x) * kTile;
    w.tile_y = (int32_t)((w.tile / a.tiles_x) % a.tiles_y) * kTile;
    w.view = w.tile / (a.tiles_x * a.tiles_y);
    // (a bin list that does not fit the buffer is not read: the host repeats the pass with a larger one)
    const uint32_t whole = (uint64_t)a.tile_offset[w.tile] + a.tile_count[w.tile] <= a.pairs_capacity ? a.tile_count[w.tile] : 0u;
    w.slot = a.heavy_slot[w.tile];
    const bool split = w.slot < a.merge_capacity;  // (~0: k_split left the list whole)
    w.parts = split ? (whole + kSplit - 1) / kSplit : 1u;
    const uint32_t first = split ? w.part * kSplit : 0u;
    w.begin = a.tile_offset[w.tile] + first;
    w.count = split ? min(kSplit, whole - min(whole, first)) : whole;
    return w.part < w.parts;
}

// The record of sequence number `seq` of `view`: an unclipped triangle sits in the slot of its work item (slot = running triangle
// number = seq / 8, view after view); the fans of clipped ones were appended and are found through the table (k_seq_table).
SAH_DEV uint32_t record_of_seq(const RasterArgs& a, uint32_t view, uint32_t seq) {
    const uint32_t total = a.counters[C_TRIS];
    uint64_t r = (uint64_t)view * total + (seq >> 3);
    if ((seq & 7u) != 0u || r >= a.record_capacity || is_empty(a.records[r])) {
        const uint64_t slot = (uint64_t)view * total * 8u + seq;
        r = slot < a.seq_capacity ? a.seq_to_record[slot] : 0u;
        if (r >= a.record_capacity) r = 0;  // only when a scratch buffer was too small: the pass is repeated
    }
    return (uint32_t)r;
}

// ---- merge cells ----------------------------------------------------------------------------------------------------------------------
// What a pass keeps per pixel across the parts of a split list: the type, the identity of its (associative) depth test, the buffer in
// global memory and the atomic that folds a part's value into it.  k_split initialises the buffers, the tile kernel folds and reads.
struct DepthCell {  // D16 code, the smallest stays (shadow cascades)
    using T = uint32_t;
    static constexpr T kClear = 0xffffu;
    static SAH_DEV T* buffer(const RasterArgs& a) { return a.merge_depth; }
    static SAH_DEV void fold(T* into, T v) { atomicMin(into, v); }
};
struct KeyCell {  // (depth key, draw order), the largest stays (G-buffer, RSM)
    using T = unsigned long long;
    static constexpr T kClear = 0ull;
    static SAH_DEV T* buffer(const RasterArgs& a) { return a.merge_keys; }
    static SAH_DEV void fold(T* into, T v) { atomicMax(into, v); }
};
struct SeqCell {  // sequence number + 1 of the latest fragment that matched the depth texel (motion vectors)
    using T = uint32_t;
    static constexpr T kClear = 0u;
    static SAH_DEV T* buffer(const RasterArgs& a) { return a.merge_seq; }
    static SAH_DEV void fold(T* into, T v) { atomicMax(into, v); }
};
// The fused G-buffer + motion pass (sah_gbuffer_motion.h) walks the same split lists twice: k_split sets up the G-buffer's cell and, in
// the same launch, the second stage's cell and tickets (a second k_split would count C_HEAVY and C_EXTRA twice).
struct KeyAndSeqCell : KeyCell {
    using Second = SeqCell;
};
template <class Merge, class = void> struct SecondCell { using type = void; };
template <class Merge> struct SecondCell<Merge, std::void_t<typename Merge::Second>> { using type = typename Merge::Second; };

// ---- targets --------------------------------------------------------------------------------------------------------------------------
// A target is what differs between the passes in the tile kernel: Merge (the cell above), Cells (the tile in LDS: merged[] plus what
// else the test reads), init (cell i before the walk), fragment (the test of a covered pixel; v = its edge functions, read by cutout
// fragments only), resolve (the finished tile -> images) and kMinWaves, the second argument of __launch_bounds__ (0: none).

// D16 shadow cascades: ds_min_u32 of the depth code.
template <bool TEX>
struct ShadowTarget {
    using Merge = DepthCell;
    static constexpr int kMinWaves = 1;
    struct Cells {
        uint32_t merged[kTile * kTile];
    };
    static SAH_DEV void init(const RasterArgs&, const TileWork&, Cells& s, uint32_t i) { s.merged[i] = Merge::kClear; }
    static SAH_DEV void fragment(const RasterArgs& a, Cells& s, const EdgeSetup& e, uint32_t rec_index, int32_t px, int32_t py, const double v[3], uint32_t cell,
                                 float z) {
        if (e.cutout) {  // shadow_masked fragment stage: discard when tinted_base_color.a <= opacity_threshold
            const ShadowAttr& sa = a.shadow_attrs[rec_index];
            float b[3], lambda[3];
            barycentrics(e, v, b);
            input_barycentrics(sa.inv_w, sa.bary, b, lambda);
            const Hn va = Hn((lambda[0] * h2f(sa.alpha[0]) + lambda[1] * h2f(sa.alpha[1])) + lambda[2] * h2f(sa.alpha[2]));
            const sah_material& m = a.materials[min(sa.material, a.num_materials - 1u)];
            Hn texel[4] = {Hn(0.f), Hn(0.f), Hn(0.f), Hn(m.base_color_texel[3])};
            const uint32_t tex = TEX ? textures_of(a, sa.material).base_color : SAH_TEXTURE_NONE;
            if (TEX && tex < a.num_textures) material_texel(a, tex, m.base_color_texel, texcoord_of(e, sa.inv_w, sa.bary, sa.uv, px, py, lambda), texel);
            const Hn alpha = texel[3] * va * Hn(m.base_color_tint[3]);
            if (tof(alpha) <= m.opacity_threshold) return;
        }
        atomicMin(&s.merged[cell], (uint32_t)__builtin_rintf(z * 65535.0f));
    }
    static SAH_DEV void resolve(const RasterArgs& a, const TileWork& w, const Cells& s) {
        // 64 texels of D16 per row = 32 dwords; 256 threads write 8 rows per step
        uint8_t* base = (uint8_t*)a.shadowmap.ptr + (size_t)w.view * a.shadowmap.slice_pitch;
        const bool pair_ok = (a.shadowmap.row_pitch % 4u) == 0 && ((uintptr_t)a.shadowmap.ptr % 4u) == 0 && (a.shadowmap.slice_pitch % 4u) == 0;
        for (uint32_t i = threadIdx.x; i < kTile * kTile / 2; i += kTileThreads) {
            const uint32_t row = i / (kTile / 2), col = (i % (kTile / 2)) * 2;
            const uint32_t px = (uint32_t)w.tile_x + col, py = (uint32_t)w.tile_y + row;
            if (py >= a.height || px >= a.width) continue;
            const uint32_t d0 = s.merged[row * kTile + col], d1 = s.merged[row * kTile + col + 1];
            uint8_t* dst = base + (size_t)py * a.shadowmap.row_pitch + (size_t)px * 2;
            if (pair_ok && px + 1 < a.width) {
                *(uint32_t*)dst = d0 | (d1 << 16);
            } else {
                *(uint16_t*)dst = (uint16_t)d0;
                if (px + 1 < a.width) *(uint16_t*)(dst + 2) = (uint16_t)d1;
            }
        }
    }
};

// G-buffer and, with a.rsm, the RSM layers: ds_max_u64 of (depth key, draw order); the winner alone is shaded.
// (the texture-sampling fragment stages are their own instantiations: 30-45 more VGPRs, which would cost the plain ones a wave per SIMD)
template <bool TEX>
struct GBufferTarget {
    using Merge = KeyCell;
    static constexpr int kMinWaves = TEX ? 1 : 3;
    struct Cells {
        unsigned long long merged[kTile * kTile];
    };
    static SAH_DEV void init(const RasterArgs&, const TileWork&, Cells& s, uint32_t i) { s.merged[i] = Merge::kClear; }
    static SAH_DEV void fragment(const RasterArgs& a, Cells& s, const EdgeSetup& e, uint32_t rec_index, int32_t px, int32_t py, const double v[3], uint32_t cell,
                                 float z) {
        // key: the larger wins.  G-buffer: reverse-Z depth bits (GREATER against the cleared 0).  RSM: D16 compare LESS against the
        // cleared 1.0, so the key holds 0xffff - code and a fragment at code 0xffff cannot pass.
        const uint32_t depth_key = a.rsm ? 0xffffu - (uint32_t)__builtin_rintf(z * 65535.0f) : __float_as_uint(z);
        if (a.rsm ? depth_key == 0u : !(z > 0.0f)) return;
        if (e.cutout) {  // alpha of tinted_base_color against the threshold (gltf_basic_pbr.slang:181-189)
            const RasterAttr& at = a.attrs[rec_index];
            float b[3], lambda[3];
            barycentrics(e, v, b);
            input_barycentrics(at.inv_w, at.bary, b, lambda);
            const sah_material& m = a.materials[min(at.material, a.num_materials - 1u)];  // k_setup validated it; the clamp only matters for stale slots of a pass that is being repeated
            Hn texel[4] = {Hn(0.f), Hn(0.f), Hn(0.f), Hn(m.base_color_texel[3])};
            const uint32_t tex = TEX ? textures_of(a, at.material).base_color : SAH_TEXTURE_NONE;
            if (TEX && tex < a.num_textures) material_texel(a, tex, m.base_color_texel, texcoord_of(e, at.inv_w, at.bary, at.uv, px, py, lambda), texel);
            const Hn alpha = texel[3] * interp_h(at, lambda, 3) * Hn(m.base_color_tint[3]);
            if (tof(alpha) <= m.opacity_threshold) return;
        }
        // low word: who wins among equal depths.  Draw order is all SOLID primitives, then all CUTOUT ones (draw_opaque, draw_masked:
        // gbuffer_phase.cpp:91-93, light_propagation_volume.cpp:611-613), triangles in list order inside a class: order = (class, seq).
        // G-buffer: a depth pre-pass (GREATER) settles the depth, the colour pass runs with compare EQUAL and depth writes off
        // (material_pipelines.cpp gbuffer_pso / gbuffer_masked_pso), so every fragment at the final depth overwrites the targets and
        // the LAST in draw order stays.  RSM: one pass, LESS with depth writes: the FIRST of equal codes stays.
        const uint32_t order = (e.cutout << 31) | e.seq;
        atomicMax(&s.merged[cell], ((unsigned long long)depth_key << 32) | (unsigned long long)(a.rsm ? ~order : order));
    }
    static SAH_DEV void resolve(const RasterArgs& a, const TileWork& w, const Cells& s) {
        // A thread's pixels are 4 rows apart in one column: consecutive ones usually belong to the same triangle, whose record,
        // varyings and material (three dependent gathers) are then kept from the previous pixel.
        const uint32_t view = w.view;
        uint32_t cached = ~0u;
        EdgeSetup e_c{};
        RasterAttr at_c{};
        sah_material m_c{};
        sah_material_textures mt_c{};
        for (uint32_t i = threadIdx.x; i < kTile * kTile; i += kTileThreads) {
            const int32_t px = w.tile_x + (int32_t)(i % kTile), py = w.tile_y + (int32_t)(i / kTile);
            if ((uint32_t)px >= a.width || (uint32_t)py >= a.height) continue;
            const unsigned long long key = s.merged[i];
            if (key == 0ull && a.rsm) {  // clear values, light_propagation_volume.cpp:586-606
                *(uint32_t*)(a.rsm_flux.ptr + (size_t)view * a.rsm_flux.slice_pitch + (size_t)py * a.rsm_flux.row_pitch + (size_t)px * 4) = 0u;
                *(uint32_t*)(a.rsm_normals.ptr + (size_t)view * a.rsm_normals.slice_pitch + (size_t)py * a.rsm_normals.row_pitch + (size_t)px * 4) = 0x00ff8080u;
                *(uint16_t*)(a.rsm_depth.ptr + (size_t)view * a.rsm_depth.slice_pitch + (size_t)py * a.rsm_depth.row_pitch + (size_t)px * 2) = 0xffffu;
            } else if (key == 0ull) {  // clear values, gbuffer_phase.cpp:66-87
                *(uint32_t*)(a.out_color.ptr + (size_t)py * a.out_color.pitch + (size_t)px * 4) = 0u;
                *(uint2*)(a.out_normals.ptr + (size_t)py * a.out_normals.pitch + (size_t)px * 8) = make_uint2(0x38003800u, 0x00003c00u);
                *(uint32_t*)(a.out_data.ptr + (size_t)py * a.out_data.pitch + (size_t)px * 4) = 0u;
                *(uint32_t*)(a.out_emission.ptr + (size_t)py * a.out_emission.pitch + (size_t)px * 4) = 0u;
                *(float*)(a.out_depth.ptr + (size_t)py * a.out_depth.pitch + (size_t)px * 4) = 0.0f;
            } else {
                const uint32_t r = record_of_seq(a, view, (a.rsm ? ~(uint32_t)key : (uint32_t)key) & 0x7fffffffu);
                if (r != cached) {
                    cached = r;
                    e_c = edge_setup(a.records[r]);
                    at_c = a.attrs[r];
                    m_c = a.materials[min(at_c.material, a.num_materials - 1u)];  // k_setup validated it; the clamp only matters for stale slots of a repeated pass
                    if (TEX) mt_c = textures_of(a, at_c.material);
                }
                if (a.rsm) shade_rsm_and_store<TEX>(a, e_c, at_c, m_c, mt_c, view, px, py, 0xffffu - (uint32_t)(key >> 32));
                else shade_and_store<TEX>(a, e_c, at_c, m_c, mt_c, px, py, __uint_as_float((uint32_t)(key >> 32)));
            }
        }
    }
};

// Motion vectors: the tile's depth texels are loaded once into LDS, a covered pixel whose fragment depth is bit-equal to its texel
// takes ds_max_u32 of the record's sequence number + 1 (compare EQUAL, no depth write: every passing fragment overwrites the target,
// so the last in draw order stays, whatever the order of the list), and the winner alone is interpolated and divided.  No textures,
// no materials, one 4-byte store per pixel.
struct MotionTarget {
    using Merge = SeqCell;
    static constexpr int kMinWaves = 0;
    struct Cells {
        uint32_t depth[kTile * kTile];
        uint32_t merged[kTile * kTile];
    };
    static SAH_DEV void init(const RasterArgs& a, const TileWork& w, Cells& s, uint32_t i) {
        const uint32_t px = (uint32_t)w.tile_x + i % kTile, py = (uint32_t)w.tile_y + i / kTile;
        // (outside the image: a pattern no clamped depth has)
        s.depth[i] = px < a.width && py < a.height ? *(const uint32_t*)(a.mv_depth.ptr + (size_t)py * a.mv_depth.pitch + (size_t)px * 4) : 0xffffffffu;
        s.merged[i] = Merge::kClear;
    }
    static SAH_DEV void fragment(const RasterArgs&, Cells& s, const EdgeSetup& e, uint32_t, int32_t, int32_t, const double*, uint32_t cell, float z) {
        if (__float_as_uint(z) == s.depth[cell]) atomicMax(&s.merged[cell], e.seq + 1u);
    }
    static SAH_DEV void resolve(const RasterArgs& a, const TileWork& w, const Cells& s) {
        uint32_t cached = ~0u;
        EdgeSetup e_c{};
        MotionAttr ma_c{};
        for (uint32_t i = threadIdx.x; i < kTile * kTile; i += kTileThreads) {
            const int32_t px = w.tile_x + (int32_t)(i % kTile), py = w.tile_y + (int32_t)(i / kTile);
            if ((uint32_t)px >= a.width || (uint32_t)py >= a.height) continue;
            uint32_t bits = 0u;  // clear value, motion_vectors_phase.cpp:90-92
            if (s.merged[i] != 0u) {
                const uint32_t r = record_of_seq(a, 0u, s.merged[i] - 1u);  // (this pass has one view)
                if (r != cached) {
                    cached = r;
                    e_c = edge_setup(a.records[r]);
                    ma_c = a.motion_attrs[r];
                }
                bits = motion_vector_of(a, e_c, ma_c, px, py);
            }
            *(uint32_t*)(a.out_motion.ptr + (size_t)py * a.out_motion.pitch + (size_t)px * 4) = bits;
        }
    }
};

// The second tile stage of the fused pass: the motion target over the G-buffer's bin lists, which also hold the CUTOUT records the
// stand-alone motion pass never sets up (scene.draw_opaque draws none of them); the walk drops them where it loads the record.
struct SharedMotionTarget : MotionTarget {
    static constexpr bool kSkipCutout = true;
};
template <class Target, class = void> constexpr bool kSkipsCutout = false;
template <class Target> constexpr bool kSkipsCutout<Target, std::void_t<decltype(Target::kSkipCutout)>> = Target::kSkipCutout;

// ---- the walk over a bin list -----------------------------------------------------------------------------------------------------------
// a covered pixel: its depth and cell, then the target's test
template <class Target>
SAH_DEV void emit_fragment(const RasterArgs& a, const TileWork& w, typename Target::Cells& s, const EdgeSetup& e, uint32_t rec_index, int32_t px, int32_t py,
                           const double v[3]) {
    Target::fragment(a, s, e, rec_index, px, py, v, (uint32_t)(py - w.tile_y) * kTile + (uint32_t)(px - w.tile_x), fragment_depth(e, px, py));
}
template <class Target>
SAH_DEV void test_pixel(const RasterArgs& a, const TileWork& w, typename Target::Cells& s, const EdgeSetup& e, uint32_t rec_index, int32_t px, int32_t py) {
    double v[3];
    if (cover(e, px, py, v)) emit_fragment<Target>(a, w, s, e, rec_index, px, py, v);
}

// One wave sweeps rows first_row, first_row + row_step, ... of 8x8 pixel blocks over the clipped bounding box (bx0, .. by1), lanes as
// the pixels of a block.  Per block the edge functions advance by one fp64 add each (exact: integers below 2^52); a block whose most
// favourable corner is outside an edge is skipped, one whose least favourable corner is inside all three needs no per-pixel coverage test.
template <class Target>
SAH_DEV void sweep(const RasterArgs& a, const TileWork& w, typename Target::Cells& s, const EdgeSetup& e, uint32_t rec_index, int32_t bx0, int32_t bx1, int32_t by1,
                   int32_t first_row, int32_t row_step, uint32_t lane) {
    const int32_t lx = (int32_t)(lane & 7u), ly = (int32_t)(lane >> 3);
    double kmax[3], kmin[3], lane_off[3], step_x[3];
    for (int i = 0; i < 3; i++) {
        kmax[i] = 7.0 * (__builtin_fmax(e.a[i], 0.0) + __builtin_fmax(e.b[i], 0.0));
        kmin[i] = 7.0 * (__builtin_fmin(e.a[i], 0.0) + __builtin_fmin(e.b[i], 0.0));
        lane_off[i] = __builtin_fma((double)lx, e.a[i], (double)ly * e.b[i]);
        step_x[i] = 8.0 * e.a[i];
    }
    for (int32_t oy = first_row; oy <= by1; oy += row_step) {
        double base[3];
        for (int i = 0; i < 3; i++) base[i] = __builtin_fma((double)oy, e.b[i], __builtin_fma((double)bx0, e.a[i], e.c[i]));
        for (int32_t ox = bx0; ox <= bx1; ox += 8) {
            bool outside = false, all_in = true;
            for (int i = 0; i < 3; i++) {
                outside = outside | (base[i] + kmax[i] < 0.0);
                all_in = all_in & (base[i] + kmin[i] > 0.0);
            }
            const int32_t px = ox + lx, py = oy + ly;
            if (!outside && px <= bx1 && py <= by1) {
                double v[3] = {0.0, 0.0, 0.0};
                bool covered = all_in;
                if (!all_in || e.cutout) {
                    covered = true;
                    for (int i = 0; i < 3; i++) {
                        v[i] = base[i] + lane_off[i];
                        covered = covered & ((v[i] > 0.0) | ((v[i] == 0.0) & (((e.tl >> i) & 1u) != 0u)));
                    }
                }
                if (covered) emit_fragment<Target>(a, w, s, e, rec_index, px, py, v);
            }
            for (int i = 0; i < 3; i++) base[i] += step_x[i];
        }
    }
}

struct BigRecord {
    EdgeSetup e;
    uint32_t rec_index;
    int32_t x0, x1, y0, y1;
};

// The part's list in rounds of 256 entries, one per thread.  A record whose bounding box covers at most kSmallArea pixels of the tile
// is walked by its own lane, up to kMediumArea by its wave; the others go to an LDS list and are rasterised by the whole workgroup,
// one after the other: lanes form an 8x8 pixel block, the four waves take alternate block rows of the bounding box.
template <class Target>
SAH_DEV void walk_list(const RasterArgs& a, const TileWork& w, typename Target::Cells& s) {
    __shared__ BigRecord s_big[kBigSlots];
    __shared__ uint32_t s_nbig;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t base = 0; base < w.count; base += kTileThreads) {
        if (tid == 0) s_nbig = 0;
        __syncthreads();
        // consecutive list entries go to different waves: a typical list is shorter than one round, and `base + tid` would hand
        // all of it to wave 0 (whose medium records are processed one after the other) while the other waves idle
        const uint32_t li = base + lane * (kTileThreads / 64u) + wave;
        uint32_t rec_index = 0, area = 0;
        int32_t x0 = 1, x1 = 0, y0 = 1, y1 = 0;
        EdgeSetup mine{};
        bool medium_rec = false;
        if (li < w.count) {
            rec_index = a.pairs[w.begin + li];
            const RasterRecord rec = a.records[rec_index];
            // (the motion stage of the fused pass drops the CUTOUT records of the shared list before any coverage work)
            if (!(kSkipsCutout<Target> && rec.cutout)) {
                x0 = max((int32_t)rec.x0, w.tile_x); x1 = min((int32_t)rec.x1, w.tile_x + kTile - 1);
                y0 = max((int32_t)rec.y0, w.tile_y); y1 = min((int32_t)rec.y1, w.tile_y + kTile - 1);
                area = (uint32_t)((x1 - x0 + 1) * (y1 - y0 + 1));
                mine = edge_setup(rec);  // every lane sets up its own record: 64 set-ups for the price of one
                medium_rec = area > kSmallArea && area <= kMediumArea;
                if (area <= kSmallArea) {
                    for (int32_t py = y0; py <= y1; py++)
                        for (int32_t px = x0; px <= x1; px++) test_pixel<Target>(a, w, s, mine, rec_index, px, py);
                } else if (area > kMediumArea) {
                    const uint32_t slot = atomicAdd(&s_nbig, 1u);
                    if (slot < kBigSlots) {
                        s_big[slot].e = mine;
                        s_big[slot].rec_index = rec_index;
                        s_big[slot].x0 = x0; s_big[slot].x1 = x1; s_big[slot].y0 = y0; s_big[slot].y1 = y1;
                    } else {
                        medium_rec = true;  // list full: the wave does it
                    }
                }
            }
        }
        // medium records: one at a time by the wave that read them, lanes as an 8x8 block sweeping the clipped bounding box; the
        // owner lane's set-up moves to scalar registers with v_readlane (no memory round trip per record)
        uint64_t medium = __ballot(medium_rec);
        while (medium) {
            const int src = __builtin_ctzll(medium);
            medium &= medium - 1;
            const uint32_t ri = readlane(rec_index, src);
            const int32_t bx0 = (int32_t)readlane((uint32_t)x0, src), bx1 = (int32_t)readlane((uint32_t)x1, src);
            const int32_t by0 = (int32_t)readlane((uint32_t)y0, src), by1 = (int32_t)readlane((uint32_t)y1, src);
            sweep<Target>(a, w, s, broadcast(mine, src), ri, bx0, bx1, by1, by0, 8, lane);
        }
        __syncthreads();
        const uint32_t nbig = min(s_nbig, kBigSlots);
        for (uint32_t k = 0; k < nbig; k++) {
            const EdgeSetup e = s_big[k].e;  // same address in every lane: an LDS broadcast
            sweep<Target>(a, w, s, e, s_big[k].rec_index, s_big[k].x0, s_big[k].x1, s_big[k].y1, s_big[k].y0 + 8 * (int32_t)wave, 8 * (int32_t)(kTileThreads / 64u), lane);
        }
        // every wave has read s_nbig / s_big of this round before thread 0 resets the counter for the next one (lists left unsplit
        // take several rounds)
        __syncthreads();
    }
}

// A split list: min / max are associative, so every part folds its tile into the tile's buffer in global memory; the part that arrives
// last (ticket) reads the merged tile back and goes on to write the images.  false: another part will.
template <class Target>
SAH_DEV bool merge_parts(const RasterArgs& a, const TileWork& w, typename Target::Cells& s) {
    using Merge = typename Target::Merge;
    __shared__ uint32_t s_last;
    typename Merge::T* merged = Merge::buffer(a) + (size_t)w.slot * (kTile * kTile);
    for (uint32_t i = threadIdx.x; i < kTile * kTile; i += kTileThreads)
        if (s.merged[i] != Merge::kClear) Merge::fold(&merged[i], s.merged[i]);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&a.tickets[w.slot], 1u) == w.parts - 1u;
    __syncthreads();
    if (!s_last) return false;
    __threadfence();
    for (uint32_t i = threadIdx.x; i < kTile * kTile; i += kTileThreads) s.merged[i] = __hip_atomic_load(&merged[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return true;
}

// ---- K5: one workgroup per tile or per part of a split list -------------------------------------------------------------------------------
template <class Target>
__global__ __launch_bounds__(kTileThreads, Target::kMinWaves) void k_raster_tiles(const RasterArgs a) {
    __shared__ typename Target::Cells s_cells;
    TileWork w;
    if (!tile_work(a, w)) return;
    for (uint32_t i = threadIdx.x; i < kTile * kTile; i += kTileThreads) Target::init(a, w, s_cells, i);
    __syncthreads();
    walk_list<Target>(a, w, s_cells);
    if (w.parts > 1 && !merge_parts<Target>(a, w, s_cells)) return;
    Target::resolve(a, w, s_cells);
}

// Cuts long bin lists into parts: a tile with more than kSplit entries gets a merge buffer (initialised here to the identity of its
// depth test), a ticket, and one extra workgroup per further part.  Tiles beyond the scratch capacity stay unsplit (slower, not wrong).
// A Merge with a Second cell (KeyAndSeqCell) also arms the second tile stage: its tickets and its buffer, under the same slots.
template <class Merge>
__global__ __launch_bounds__(256) void k_split(const RasterArgs a) {
    using Second = typename SecondCell<Merge>::type;
    const uint32_t ntiles = a.tiles_x * a.tiles_y * a.num_views;
    const uint32_t tile = blockIdx.x;  // one workgroup per tile: the merge buffer of a heavy tile is initialised by all 256 threads
    __shared__ uint32_t s_slot;
    if (tile >= ntiles) return;
    if (threadIdx.x == 0) {
        uint32_t slot = ~0u;
        const uint32_t count = a.tile_count[tile];
        if (count > kSplit && (uint64_t)a.tile_offset[tile] + count <= a.pairs_capacity) {
            const uint32_t parts = (count + kSplit - 1) / kSplit;
            const uint32_t h = atomicAdd(&a.counters[C_HEAVY], 1u);
            if (h < a.merge_capacity) {
                const uint32_t e = atomicAdd(&a.counters[C_EXTRA], parts - 1u);
                if ((uint64_t)e + parts - 1u <= a.extra_capacity) {
                    slot = h;
                    a.tickets[h] = 0u;
                    if constexpr (!std::is_void_v<Second>) a.motion_tickets[h] = 0u;
                    for (uint32_t p = 1; p < parts; p++) a.extra_parts[e + p - 1u] = make_uint2(tile, p);
                }
            }
        }
        a.heavy_slot[tile] = slot;
        s_slot = slot;
    }
    __syncthreads();
    if (s_slot == ~0u) return;
    typename Merge::T* merged = Merge::buffer(a) + (size_t)s_slot * (kTile * kTile);
    for (uint32_t i = threadIdx.x; i < kTile * kTile; i += 256) merged[i] = Merge::kClear;
    if constexpr (!std::is_void_v<Second>) {
        typename Second::T* second = Second::buffer(a) + (size_t)s_slot * (kTile * kTile);
        for (uint32_t i = threadIdx.x; i < kTile * kTile; i += 256) second[i] = Second::kClear;
    }
}

// seq -> record index for the appended records (fans of clipped triangles; G-buffer resolve)
__global__ __launch_bounds__(256) void k_seq_table(const RasterArgs a) {
    const uint32_t nrec = record_count(a), first = a.counters[C_TRIS] * a.num_views;
    for (uint32_t r = first + blockIdx.x * 256 + threadIdx.x; r < nrec; r += gridDim.x * 256)
    {
        const uint64_t slot = (uint64_t)a.records[r].view * a.counters[C_TRIS] * 8u + a.records[r].seq;
        if (slot < a.seq_capacity) a.seq_to_record[slot] = r;
    }
}

template <class Target, class Split = typename Target::Merge>
void launch_tile_kernels(const RasterArgs& a, uint32_t ntiles, hipStream_t st) {
    // every tile gets its heavy_slot (~0 when its list stays whole), also for an empty scene
    hipLaunchKernelGGL(k_split<Split>, dim3(ntiles), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_raster_tiles<Target>, dim3(ntiles + a.extra_capacity), dim3(kTileThreads), 0, st, a);
}
// The second tile stage of the fused pass: the same bin lists, heavy_slot and extra_parts; the tickets k_split armed for it.  Stream
// order makes the depth plane the first stage wrote visible to it.
void launch_shared_motion_tiles(const RasterArgs& a, uint32_t ntiles, hipStream_t st) {
    RasterArgs m = a;
    m.tickets = a.motion_tickets;
    hipLaunchKernelGGL(k_raster_tiles<SharedMotionTarget>, dim3(ntiles + a.extra_capacity), dim3(kTileThreads), 0, st, m);
}

// ---- translucent geometry over the lit scene (sah_translucent.h) ------------------------------------------------------------------------
// Blending needs every fragment of a pixel, in draw order, where the cells above keep one winner.  One workgroup per tile peels its bin
// list by sequence number: round k walks the WHOLE list (walk_list and sweep as they are) and keeps, per pixel, the smallest seq + 1 above
// the one blended in round k - 1 among the fragments that pass the depth test — ds_min_u32, so the order of the list does not show —; the
// resolve of the round rebuilds that fragment's texel (fragment_stage, the G-buffer's own), lights it with the general
// restatement of sah_lighting (shade_pixel_general: no new shading arithmetic) and blends it into `lit`.  The workgroup owns its tile's
// pixels: no global atomics.  Rounds end when no pixel of the tile found a fragment; a tile costs (list length) x (deepest pixel).
// Lists are never split: a peel cannot be merged across workgroups without a barrier per layer.
struct TranslucentTarget {
    struct Cells {
        uint32_t depth[kTile * kTile];   // the opaque depth texel's bits; a NaN for the pixels this call does not write
        uint32_t done[kTile * kTile];    // seq + 1 of the fragment taken in the last round (0: none yet)
        uint32_t merged[kTile * kTile];  // this round's: the smallest seq + 1 above `done` (~0: none)
        uint16_t blended[kTile * kTile]; // fragments blended so far (statistics word 7), saturating
    };
    static SAH_DEV void fragment(const RasterArgs&, Cells& s, const EdgeSetup& e, uint32_t, int32_t, int32_t, const double*, uint32_t cell, float z) {
        // reverse-Z GREATER, strict, no depth write; a NaN on either side compares false
        if (z > __uint_as_float(s.depth[cell]) && e.seq + 1u > s.done[cell]) atomicMin(&s.merged[cell], e.seq + 1u);
    }
};

// Blending is not idempotent, and the host repeats a pass whose scratch buffers were too small or fails one with a bad texture table
// (api_raster.cpp: run): the tile stage of such an attempt must leave `lit` alone.  Every count the host will look at is final before this
// stage starts, so the workgroups decide as the host will.
SAH_DEV bool translucent_attempt_counts(const RasterArgs& a) {
    const uint64_t tris = a.counters[C_TRIS];
    return tris < (1u << 28) && a.counters[C_BAD_TEXTURE] == 0u && tris + a.counters[C_RECORDS] <= a.record_capacity &&
           a.counters[C_CLIPPED] <= a.clip_capacity && a.counters[C_PAIRS] <= a.pairs_capacity && tris * 8u + 1u <= a.seq_capacity;
}

template <int SUN, int GI, bool TEX>
__global__ __launch_bounds__(kTileThreads) void k_translucent_tiles(const RasterArgs a, const LightingArgs la, const CsmArgs csm, const LpvArgs lpv) {
    __shared__ TranslucentTarget::Cells s;
    __shared__ float s_lut[512];
    __shared__ uint32_t s_deepest;
    if (!translucent_attempt_counts(a)) return;
    TileWork w;
    w.tile = blockIdx.x;
    w.part = 0;
    w.parts = 1;
    w.slot = ~0u;
    w.view = 0;
    w.tile_x = (int32_t)(w.tile % a.tiles_x) * kTile;
    w.tile_y = (int32_t)(w.tile / a.tiles_x) * kTile;
    w.begin = a.tile_offset[w.tile];
    w.count = a.tile_count[w.tile];
    // nothing to draw in this tile, or none of its rows in the range: no plane is read or written
    if (w.count == 0u || (uint32_t)w.tile_y >= la.row_end || (uint32_t)w.tile_y + kTile <= la.row_begin) return;
    for (uint32_t i = threadIdx.x; i < kTile * kTile; i += kTileThreads) {
        const uint32_t px = (uint32_t)w.tile_x + i % kTile, py = (uint32_t)w.tile_y + i / kTile;
        const bool mine = px < a.width && py >= la.row_begin && py < la.row_end;  // (row_end <= height)
        s.depth[i] = mine ? *(const uint32_t*)(la.depth.ptr + (size_t)py * la.depth.pitch + (size_t)px * 4) : 0xffffffffu;
        s.done[i] = 0u;
        s.merged[i] = ~0u;
        s.blended[i] = 0;
    }
    for (uint32_t i = threadIdx.x; i < 512u; i += kTileThreads) s_lut[i] = la.luts[i];
    if (threadIdx.x == 0) s_deepest = 0u;
    __syncthreads();
    const SkyArgs sky{};  // (a fragment is a surface: the sky fill is compiled out)
    uint32_t deepest = 0u;
    for (;;) {
        walk_list<TranslucentTarget>(a, w, s);  // (ends with a barrier)
        bool found = false;
        uint32_t cached = ~0u;
        EdgeSetup e_c{};
        RasterAttr at_c{};
        sah_material m_c{};
        sah_material_textures mt_c{};
#pragma unroll 1
        for (uint32_t i = threadIdx.x; i < kTile * kTile; i += kTileThreads) {
            const uint32_t taken = s.merged[i];
            if (taken == ~0u) continue;
            found = true;
            s.done[i] = taken;
            s.merged[i] = ~0u;
            const int32_t px = w.tile_x + (int32_t)(i % kTile), py = w.tile_y + (int32_t)(i / kTile);
            const uint32_t r = record_of_seq(a, 0u, taken - 1u);
            if (r != cached) {
                cached = r;
                e_c = edge_setup(a.records[r]);
                at_c = a.attrs[r];
                m_c = a.materials[min(at_c.material, a.num_materials - 1u)];
                if (TEX) mt_c = textures_of(a, at_c.material);
            }
            Px p;  // the fragment's texel as the G-buffer would hold it
            fragment_stage<TEX>(a, e_c, at_c, m_c, mt_c, px, py, [&](uint32_t color_bits, uint2 nbits, uint32_t data_bits, uint32_t emission_bits) {
                p.color = color_bits;
                p.data = data_bits;
                p.emission = emission_bits;
                p.n01 = nbits.x;
                p.n23 = nbits.y;
            });
            const uint32_t code = p.color >> 24;
            if (code == 0u) continue;  // alpha 0: skipped, not blended
            p.depth = fragment_depth(e_c, px, py);
            p.ao = 1.0f;
            p.mask = 1.0f;
            const uint2 src = shade_pixel_general<SUN, GI, false>(la, csm, lpv, sky, (uint32_t)px, (uint32_t)py, p, s_lut);
            uint2* at = (uint2*)(const_cast<uint8_t*>(la.lit.ptr) + (size_t)py * la.lit.pitch + (size_t)px * 8);
            const uint2 dst = *at;
            // SRC_ALPHA / ONE_MINUS_SRC_ALPHA on colour and alpha alike, every operator rounded in fp32, stored as Lighting stores
            const float alpha = s_lut[256u + code], rest = 1.0f - alpha;
            const uint32_t sw[2] = {src.x, src.y}, dw[2] = {dst.x, dst.y};
            uint32_t ow[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const float lo = h2f((uint16_t)sw[k]) * alpha + h2f((uint16_t)dw[k]) * rest;
                const float hi = h2f((uint16_t)(sw[k] >> 16)) * alpha + h2f((uint16_t)(dw[k] >> 16)) * rest;
                ow[k] = (uint32_t)f2h(lo) | ((uint32_t)f2h(hi) << 16);
            }
            *at = make_uint2(ow[0], ow[1]);
            const uint32_t n = min((uint32_t)s.blended[i] + 1u, 0xffffu);
            s.blended[i] = (uint16_t)n;
            deepest = max(deepest, n);
        }
        if (!__syncthreads_or(found)) break;
    }
    if (deepest) atomicMax(&s_deepest, deepest);
    __syncthreads();
    if (threadIdx.x == 0 && s_deepest) atomicMax(&a.counters[C_STATS + 7], s_deepest);
}

template <int SUN, int GI>
void launch_translucent(const RasterArgs& a, const TranslucentShade& t, uint32_t ntiles, hipStream_t st) {
    if (a.textures) hipLaunchKernelGGL((k_translucent_tiles<SUN, GI, true>), dim3(ntiles), dim3(kTileThreads), 0, st, a, t.lighting, t.csm, t.lpv);
    else hipLaunchKernelGGL((k_translucent_tiles<SUN, GI, false>), dim3(ntiles), dim3(kTileThreads), 0, st, a, t.lighting, t.csm, t.lpv);
}

}  // namespace

// Stage 2 of the translucent pass: the bins, the sequence table, then the peel.  The list of every tile is walked whole (no k_split).
hipError_t launch_translucent_tiles(const RasterArgs& a, const TranslucentShade& t, hipStream_t st) {
    const uint32_t ntiles = a.tiles_x * a.tiles_y;
    if (a.num_primitives == 0) return hipSuccess;
    launch_raster_fill_bins(a, st);
    hipLaunchKernelGGL(k_seq_table, dim3(64), dim3(256), 0, st, a);
    const bool csm = t.sun_mode == SAH_SHADOW_MODE_CSM, lpv = t.gi_kind == SAH_GI_LPV;
    if (csm && lpv) launch_translucent<SAH_SHADOW_MODE_CSM, SAH_GI_LPV>(a, t, ntiles, st);
    else if (csm) launch_translucent<SAH_SHADOW_MODE_CSM, SAH_GI_NONE>(a, t, ntiles, st);
    else if (lpv) launch_translucent<SAH_SHADOW_MODE_OFF, SAH_GI_LPV>(a, t, ntiles, st);
    else launch_translucent<SAH_SHADOW_MODE_OFF, SAH_GI_NONE>(a, t, ntiles, st);
    return hipGetLastError();
}


// Stage 2: fill the bins, rasterise and write the images.
hipError_t launch_raster_tiles(const RasterArgs& a, hipStream_t st) {
    const uint32_t ntiles = a.tiles_x * a.tiles_y * a.num_views;
    if (a.num_primitives) {
        launch_raster_fill_bins(a, st);
        if (a.pass != RasterPass::Shadow) hipLaunchKernelGGL(k_seq_table, dim3(64), dim3(256), 0, st, a);
    }
    switch (a.pass) {
        case RasterPass::Shadow:
            if (a.textures && a.shadow_attrs) launch_tile_kernels<ShadowTarget<true>>(a, ntiles, st);
            else launch_tile_kernels<ShadowTarget<false>>(a, ntiles, st);
            break;
        case RasterPass::GBuffer:
        case RasterPass::Rsm:
            if (a.textures) launch_tile_kernels<GBufferTarget<true>>(a, ntiles, st);
            else launch_tile_kernels<GBufferTarget<false>>(a, ntiles, st);
            break;
        case RasterPass::Motion: launch_tile_kernels<MotionTarget>(a, ntiles, st); break;
        case RasterPass::GBufferMotion:
            if (a.textures) launch_tile_kernels<GBufferTarget<true>, KeyAndSeqCell>(a, ntiles, st);
            else launch_tile_kernels<GBufferTarget<false>, KeyAndSeqCell>(a, ntiles, st);
            launch_shared_motion_tiles(a, ntiles, st);
            break;
        case RasterPass::Translucent: break;  // (its tile stage needs the Lighting blocks: launch_translucent_tiles)
    }
    return hipGetLastError();
}

}  // namespace sah
