// C ABI: the scene rasteriser (sun shadow cascades, depth + G-buffer) — argument checks, scratch buffers, the two launch stages.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/sah_hip.h"
#include "../../include/sah_gbuffer_motion.h"
#include "../../include/sah_motion_vectors.h"
#include "../../include/sah_translucent.h"
#include "ctx.hpp"
#include "launch.hpp"
#include "lighting_stages.hpp"

namespace {
constexpr uint32_t kTile = sah::kRasterTile;
constexpr uint32_t kMaxExtent = 8192;  // keeps every snapped coordinate inside the guard band below 2^24.1
enum Scratch { S_COUNTERS, S_TRI_BASE, S_RECORDS, S_ATTRS, S_TILES, S_PAIRS, S_SEQ, S_CLIPQ, S_VPL_CELLS, S_VPL_CANDIDATES, S_HEAVY, S_EXTRA, S_TICKETS, S_MERGE, S_MOTION };

int ensure(sah_ctx* ctx, int slot, size_t bytes) {
    SahBuffer& b = ctx->raster.buf[slot];
    if (b.bytes >= bytes && b.ptr) return SAH_OK;
    b.release();
    const size_t want = bytes + bytes / 4 + 256;
    HIP_TRY(ctx, hipMalloc(&b.ptr, want));
    b.bytes = want;
    return SAH_OK;
}

// fp16 bit pattern -> sRGB8 code of an R8G8B8A8_SRGB store: the OETF evaluated in fp64 and rounded to fp32, then UNORM8 as
// floor(s * 255 + 0.5) in fp32 (DESIGN.md §3 "stores")
int ensure_srgb_table(sah_ctx* ctx) {
    if (ctx->raster.half_to_srgb8) return SAH_OK;
    std::vector<uint8_t> table(65536);
    for (uint32_t bits = 0; bits < 65536; bits++) {
        const uint32_t sign = bits >> 15, ex = (bits >> 10) & 31u, man = bits & 1023u;
        double v;
        if (ex == 31) v = man ? NAN : INFINITY;
        else if (ex == 0) v = std::ldexp((double)man, -24);
        else v = std::ldexp((double)(man | 1024u), (int)ex - 25);
        if (sign) v = -v;
        uint8_t code = 0;
        if (v > 0.0) {  // NaN and non-positive values encode to 0
            if (v >= 1.0) code = 255;
            else {
                const float s = (float)((v <= 0.0031308) ? 12.92 * v : 1.055 * std::pow(v, 1.0 / 2.4) - 0.055);
                code = !(s > 0.0f) ? 0 : (s >= 1.0f ? 255 : (uint8_t)(s * 255.0f + 0.5f));
            }
        }
        table[bits] = code;
    }
    HIP_TRY(ctx, hipMalloc((void**)&ctx->raster.half_to_srgb8, 65536));
    HIP_TRY(ctx, hipMemcpy(ctx->raster.half_to_srgb8, table.data(), 65536, hipMemcpyHostToDevice));
    return SAH_OK;
}

bool geometry_ok(const sah_scene_geometry* g, bool need_attributes) {
    if (!g) return false;
    if (g->num_primitives == 0) return true;
    if (!g->primitives || !g->indices || !g->vertex_positions) return false;
    if (need_attributes && (!g->vertex_data || !g->materials || g->num_materials == 0)) return false;
    return g->num_primitives < (1u << 24);
}

// What the scratch of a pass looks like (raster_args.hpp: RasterPass).
struct PassScratch {
    struct {
        int slot;      // a buffer that holds one attribute record per raster record
        size_t bytes;  // ... of this size; 0: none
    } attr[2];         // every pass but the fused one has one kind of attribute record
    size_t cell_bytes[2];  // per pixel of a split tile's merge buffer, per tile stage (the second: 0 unless the pass has two)
    bool seq_table;        // the resolve looks records up by sequence number
};
PassScratch scratch_of(sah::RasterPass pass, const sah_scene_geometry* scene) {
    switch (pass) {
        case sah::RasterPass::Shadow: {
            // the alpha test of CUTOUT primitives needs their vertex colours and materials (lean records, raster_args.hpp)
            const bool attrs = scene->vertex_data && scene->materials && scene->num_materials;
            return {{{S_ATTRS, attrs ? sizeof(sah::ShadowAttr) : 0}, {S_MOTION, 0}}, {sizeof(uint32_t), 0}, false};
        }
        case sah::RasterPass::GBuffer:
        case sah::RasterPass::Rsm: return {{{S_ATTRS, sizeof(sah::RasterAttr)}, {S_MOTION, 0}}, {sizeof(unsigned long long), 0}, true};
        // the motion-vectors pass carries its varying in records of its own; the G-buffer's attributes stay as they are
        case sah::RasterPass::Motion: return {{{S_MOTION, sizeof(sah::MotionAttr)}, {S_ATTRS, 0}}, {sizeof(uint32_t), 0}, true};
        // the fused pass owns both attribute buffers, and a merge cell and a ticket per tile stage
        case sah::RasterPass::GBufferMotion:
            return {{{S_ATTRS, sizeof(sah::RasterAttr)}, {S_MOTION, sizeof(sah::MotionAttr)}}, {sizeof(unsigned long long), sizeof(uint32_t)}, true};
        // the translucent pass peels its lists whole: no merge cells
        case sah::RasterPass::Translucent: return {{{S_ATTRS, sizeof(sah::RasterAttr)}, {S_MOTION, 0}}, {0, 0}, true};
    }
    return {};
}

// Runs both stages; grows the scratch buffers and repeats the pass when a guess was too small.
int run(sah_ctx* ctx, sah::RasterArgs& a, const sah_scene_geometry* scene, sah::RasterPass pass, uint32_t* stats, const sah::TranslucentShade* translucent = nullptr) {
    using namespace sah;  // Counter
    auto& r = ctx->raster;
    a.pass = pass;
    a.rsm = pass == RasterPass::Rsm;
    const PassScratch ps = scratch_of(pass, scene);
    const uint32_t ntiles = a.tiles_x * a.tiles_y * a.num_views;
    if (!r.host_counters) HIP_TRY(ctx, hipHostMalloc((void**)&r.host_counters, C_WORDS * sizeof(uint32_t)));
    if (int rc = ensure(ctx, S_COUNTERS, C_WORDS * sizeof(uint32_t)); rc != SAH_OK) return rc;
    if (int rc = ensure(ctx, S_TRI_BASE, (size_t)(scene->num_primitives + 1) * sizeof(uint32_t)); rc != SAH_OK) return rc;
    if (int rc = ensure(ctx, S_TILES, (size_t)ntiles * 3 * sizeof(uint32_t)); rc != SAH_OK) return rc;
    // First guesses: every index triple is drawn once per view and survives (instanced index ranges or clipping can exceed it); the
    // bin list and the draw-order table as large as the last call needed.  Both stages are launched back to back and the counters are
    // read once, at the end: if any buffer turned out too small (the kernels never write past a buffer, they only count), it is grown
    // and the pass repeated.  From the second frame of a scene on this is one iteration with no idle gap on the GPU.
    size_t want_records = (size_t)(scene->num_indices / 3) * a.num_views + 1024, want_clipped = want_records / 8 + 1024;
    size_t want_pairs = std::max<size_t>(r.buf[S_PAIRS].bytes / sizeof(uint32_t), 2 * want_records + 4 * (size_t)ntiles);
    size_t want_seq = ps.seq_table ? std::max<size_t>(r.buf[S_SEQ].bytes / sizeof(uint32_t), (size_t)(scene->num_indices / 3) * 8 * a.num_views + 64) : 0;
    for (int attempt = 0; attempt < 4; attempt++) {
        if (int rc = ensure(ctx, S_CLIPQ, want_clipped * sizeof(uint2)); rc != SAH_OK) return rc;
        if (int rc = ensure(ctx, S_RECORDS, want_records * sizeof(RasterRecord)); rc != SAH_OK) return rc;
        for (const auto& at : ps.attr)
            if (at.bytes)
                if (int rc = ensure(ctx, at.slot, want_records * at.bytes); rc != SAH_OK) return rc;
        if (int rc = ensure(ctx, S_PAIRS, want_pairs * sizeof(uint32_t)); rc != SAH_OK) return rc;
        if (ps.seq_table)
            if (int rc = ensure(ctx, S_SEQ, want_seq * sizeof(uint32_t)); rc != SAH_OK) return rc;
        a.clip_queue = (uint2*)r.buf[S_CLIPQ].ptr;
        a.clip_capacity = (uint32_t)std::min<size_t>(r.buf[S_CLIPQ].bytes / sizeof(uint2), 0xffffffffu);
        a.counters = (uint32_t*)r.buf[S_COUNTERS].ptr;
        a.tri_base = (uint32_t*)r.buf[S_TRI_BASE].ptr;
        a.records = (RasterRecord*)r.buf[S_RECORDS].ptr;
        a.record_capacity = (uint32_t)std::min<size_t>(r.buf[S_RECORDS].bytes / sizeof(RasterRecord), 0xffffffffu);
        for (const auto& at : ps.attr)
            if (at.bytes) a.record_capacity = (uint32_t)std::min<size_t>(a.record_capacity, r.buf[at.slot].bytes / at.bytes);
        const bool gbuffer_cells = pass == RasterPass::GBuffer || pass == RasterPass::Rsm || pass == RasterPass::GBufferMotion;
        const bool motion_cells = pass == RasterPass::Motion || pass == RasterPass::GBufferMotion;
        a.attrs = (RasterAttr*)r.buf[S_ATTRS].ptr;  // (read by the G-buffer, RSM and fused passes only)
        a.shadow_attrs = pass == RasterPass::Shadow && ps.attr[0].bytes ? (ShadowAttr*)r.buf[S_ATTRS].ptr : nullptr;
        a.motion_attrs = motion_cells ? (MotionAttr*)r.buf[S_MOTION].ptr : nullptr;
        a.tile_count = (uint32_t*)r.buf[S_TILES].ptr;
        a.tile_cursor = a.tile_count + ntiles;
        a.tile_offset = a.tile_count + 2 * (size_t)ntiles;
        a.pairs = (uint32_t*)r.buf[S_PAIRS].ptr;
        a.pairs_capacity = (uint32_t)std::min<size_t>(r.buf[S_PAIRS].bytes / sizeof(uint32_t), 0xffffffffu);
        a.seq_to_record = (uint32_t*)r.buf[S_SEQ].ptr;
        a.seq_capacity = ps.seq_table ? r.buf[S_SEQ].bytes / sizeof(uint32_t) : 0;
        // long bin lists are cut into parts of kRasterSplit entries: at most pairs / kRasterSplit further parts, and a merge buffer per split tile (the
        // number of those is capped: tiles beyond it are processed whole)
        a.extra_capacity = a.pairs_capacity / kRasterSplit + 1u;
        a.merge_capacity = std::min<uint32_t>(a.extra_capacity, ctx->raster_merge_cap);
        if (int rc = ensure(ctx, S_HEAVY, (size_t)ntiles * sizeof(uint32_t)); rc != SAH_OK) return rc;
        if (int rc = ensure(ctx, S_EXTRA, (size_t)a.extra_capacity * sizeof(uint2)); rc != SAH_OK) return rc;
        const size_t stages = ps.cell_bytes[1] ? 2 : 1, slot_cells = (size_t)a.merge_capacity * kTile * kTile;
        if (int rc = ensure(ctx, S_TICKETS, stages * a.merge_capacity * sizeof(uint32_t)); rc != SAH_OK) return rc;
        if (int rc = ensure(ctx, S_MERGE, slot_cells * (ps.cell_bytes[0] + ps.cell_bytes[1])); rc != SAH_OK) return rc;
        a.heavy_slot = (uint32_t*)r.buf[S_HEAVY].ptr;
        a.extra_parts = (uint2*)r.buf[S_EXTRA].ptr;
        a.tickets = (uint32_t*)r.buf[S_TICKETS].ptr;
        // one buffer, typed by the pass's merge cell; the second tile stage of the fused pass has its cells behind the first's and
        // its tickets behind the first's
        a.merge_depth = pass == RasterPass::Shadow ? (uint32_t*)r.buf[S_MERGE].ptr : nullptr;
        a.merge_keys = gbuffer_cells ? (unsigned long long*)r.buf[S_MERGE].ptr : nullptr;
        a.merge_seq = motion_cells ? (uint32_t*)((uint8_t*)r.buf[S_MERGE].ptr + (stages == 2 ? slot_cells * ps.cell_bytes[0] : 0)) : nullptr;
        a.motion_tickets = stages == 2 ? a.tickets + a.merge_capacity : nullptr;
        HIP_TRY(ctx, launch_raster_setup(a, ctx->stream));
        // (the translucent tile stage blends, so it must not run twice: its workgroups look at the counts themselves and leave the lit image
        //  alone in an attempt that the code below will repeat or fail — raster_tiles.hip: translucent_attempt_counts)
        if (translucent) HIP_TRY(ctx, launch_translucent_tiles(a, *translucent, ctx->stream));
        else HIP_TRY(ctx, launch_raster_tiles(a, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(r.host_counters, a.counters, C_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t report[4] = {(uint32_t)attempt + 1u, a.record_capacity, a.clip_capacity, a.pairs_capacity};
        std::memcpy(r.last_pass, report, sizeof(report));
        const uint32_t* hc = r.host_counters;
        const size_t total_tris = hc[C_TRIS], clipped = hc[C_CLIPPED], pairs = hc[C_PAIRS];
        if (total_tris >= (1u << 28)) return fail(ctx, SAH_ERR_UNSUPPORTED, "rasteriser: more than 2^28 triangles in one pass");
        if (hc[C_BAD_TEXTURE])
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rasteriser: %u invalid texture slots or bindings (index beyond the table, more than %d levels, a level "
                        "that is not R8G8B8A8_UNORM / _SRGB, a sampler enum out of range)", hc[C_BAD_TEXTURE], SAH_MAX_TEXTURE_MIPS);
        if (hc[C_CUTOUT_NO_ATTR])
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "shadow_render: the scene has CUTOUT primitives (%u triangles): vertex_data and materials are needed "
                        "for their alpha test (shadow_masked pipeline)", hc[C_CUTOUT_NO_ATTR]);
        // records: one slot per (view, triangle) plus the appended fans of the clipped ones
        const size_t need_records = total_tris * a.num_views + hc[C_RECORDS];
        const size_t need_seq = ps.seq_table ? total_tris * 8 * a.num_views + 1 : 0;
        if (need_records <= a.record_capacity && clipped <= a.clip_capacity && pairs <= a.pairs_capacity && need_seq <= a.seq_capacity) break;
        if (attempt == 3) return fail(ctx, SAH_ERR_HIP, "rasteriser: scratch buffers still too small after regrowing");
        // a short clip queue hides records and a short record buffer hides bin entries: size for the worst case of what was seen
        want_clipped = std::max<size_t>(want_clipped, clipped);
        want_records = std::max<size_t>(want_records, need_records + 7 * clipped);
        want_pairs = std::max<size_t>(want_pairs, pairs + pairs / 4 + 16);
        want_seq = std::max<size_t>(want_seq, need_seq);
    }
    if (stats) HIP_TRY(ctx, hipMemcpyAsync(stats, a.counters + C_STATS, SAH_RASTER_STATS_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    return SAH_OK;
}

// the extent of every view of a pass and what follows from it
void fill_extent(sah::RasterArgs& a, uint32_t width, uint32_t height) {
    a.width = width;
    a.height = height;
    a.half_w = (float)width * 0.5f;
    a.half_h = (float)height * 0.5f;
    a.tiles_x = (width + kTile - 1) / kTile;
    a.tiles_y = (height + kTile - 1) / kTile;
}

void fill_scene(sah_ctx* ctx, sah::RasterArgs& a, const sah_scene_geometry* scene) {
    a.luts = ctx->luts;
    a.positions = scene->vertex_positions;
    a.vertex_data = scene->vertex_data;
    a.indices = scene->indices;
    a.primitives = scene->primitives;
    a.materials = scene->materials;
    a.num_primitives = scene->num_primitives;
    a.num_indices = scene->num_indices;
    a.num_vertices = scene->num_vertices;
    a.num_materials = scene->num_materials;
    const bool textured = scene->textures && scene->material_textures && scene->num_textures;
    a.textures = textured ? scene->textures : nullptr;
    a.material_textures = textured ? scene->material_textures : nullptr;
    a.num_textures = textured ? scene->num_textures : 0;
    a.shader_mip_bias = 0.0f;
}

// the five targets of a G-buffer pass: format, the depth plane's extent, alignment; null: all are fine
const char* bad_gbuffer_target(const sah_gbuffer* out, uint32_t W, uint32_t H) {
    const struct { const sah_plane* p; uint32_t fmt; uint32_t align; const char* name; } targets[5] = {
        {&out->color, SAH_FORMAT_R8G8B8A8_SRGB, 4, "color"},   {&out->normals, SAH_FORMAT_R16G16B16A16_SFLOAT, 8, "normals"},
        {&out->data, SAH_FORMAT_R8G8B8A8_UNORM, 4, "data"},    {&out->emission, SAH_FORMAT_R8G8B8A8_SRGB, 4, "emission"},
        {&out->depth, SAH_FORMAT_D32_SFLOAT, 4, "depth"}};
    for (const auto& t : targets)
        if (!plane_ok(t.p, t.fmt, t.fmt, W, H) || ((uintptr_t)t.p->ptr % t.align) || (t.p->row_pitch_bytes % t.align)) return t.name;
    return nullptr;
}
bool motion_target_ok(const sah_plane* motion_vectors, uint32_t W, uint32_t H) {
    return plane_ok(motion_vectors, SAH_FORMAT_R16G16_SFLOAT, SAH_FORMAT_R16G16_SFLOAT, W, H) && !((uintptr_t)motion_vectors->ptr % 4) &&
           !(motion_vectors->row_pitch_bytes % 4);
}

// what a G-buffer pass takes from its view and its targets
void fill_gbuffer(sah_ctx* ctx, sah::RasterArgs& a, const sah_view_data* view, const sah_gbuffer* out) {
    a.num_views = 1;
    a.shader_mip_bias = view->material_texture_mip_bias;
    std::memcpy(a.view_matrix, view->view, 64);
    std::memcpy(a.clip_matrix[0], view->projection, 64);
    fill_extent(a, out->depth.width, out->depth.height);
    a.half_to_srgb8 = ctx->raster.half_to_srgb8;
    a.out_color = parg(&out->color);
    a.out_normals = parg(&out->normals);
    a.out_data = parg(&out->data);
    a.out_emission = parg(&out->emission);
    a.out_depth = parg(&out->depth);
}
// what a motion-vectors pass takes from its view and its planes beyond the extent and this frame's matrices
void fill_motion(sah::RasterArgs& a, const sah_view_data* view, const sah_plane* depth, const sah_plane* motion_vectors) {
    std::memcpy(a.prev_view_matrix, view->last_frame_view, 64);
    std::memcpy(a.prev_clip_matrix, view->last_frame_projection, 64);
    a.render_resolution[0] = view->render_resolution[0];
    a.render_resolution[1] = view->render_resolution[1];
    a.mv_depth = parg(depth);
    a.out_motion = parg(motion_vectors);
}
}  // namespace

extern "C" {

int sah_shadow_render(sah_ctx* ctx, const sah_scene_geometry* scene, const sah_sun_light_constants* sun, uint32_t num_cascades,
                      const sah_volume* shadowmap, uint32_t* stats) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!geometry_ok(scene, false) || !sun || num_cascades == 0 || num_cascades > 4) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "shadow_render: bad scene or cascade count");
    if (!shadowmap || !shadowmap->ptr || shadowmap->format != SAH_FORMAT_D16_UNORM) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "shadow_render: the shadow map must be D16_UNORM");
    if (shadowmap->width == 0 || shadowmap->height == 0 || shadowmap->width > kMaxExtent || shadowmap->height > kMaxExtent || shadowmap->depth < num_cascades ||
        (uint64_t)shadowmap->row_pitch_bytes < (uint64_t)shadowmap->width * 2 || (uint64_t)shadowmap->slice_pitch_bytes < (uint64_t)shadowmap->row_pitch_bytes * shadowmap->height ||
        ((uintptr_t)shadowmap->ptr % 2) || (shadowmap->row_pitch_bytes % 2) || (shadowmap->slice_pitch_bytes % 2))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "shadow_render: shadow map extent (1..%u), layers or pitches", kMaxExtent);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_raster));
    sah::RasterArgs a{};
    fill_scene(ctx, a, scene);
    a.num_views = num_cascades;
    for (uint32_t c = 0; c < num_cascades; c++) std::memcpy(a.clip_matrix[c], sun->cascade_matrices[c], 64);
    fill_extent(a, shadowmap->width, shadowmap->height);
    a.shadowmap = varg(*shadowmap);
    return run(ctx, a, scene, sah::RasterPass::Shadow, stats);
}

int sah_gbuffer_render(sah_ctx* ctx, const sah_scene_geometry* scene, const sah_view_data* view, const sah_gbuffer* out, uint32_t* stats) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!geometry_ok(scene, true) || !view || !out) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "gbuffer_render: bad scene, view or targets");
    const uint32_t W = out->depth.width, H = out->depth.height;
    if (W == 0 || H == 0 || W > kMaxExtent || H > kMaxExtent) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "gbuffer_render: extent must be 1..%u", kMaxExtent);
    if (const char* name = bad_gbuffer_target(out, W, H))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "gbuffer_render: target '%s' has the wrong format, extent or alignment", name);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_raster));
    if (int rc = ensure_srgb_table(ctx); rc != SAH_OK) return rc;
    sah::RasterArgs a{};
    fill_scene(ctx, a, scene);
    fill_gbuffer(ctx, a, view, out);
    return run(ctx, a, scene, sah::RasterPass::GBuffer, stats);
}

// sah_gbuffer_motion.h: sah_gbuffer_render, then sah_motion_vectors_render against the depth it wrote, with one set-up, one set of bin
// lists and one read-back of the counters
int sah_gbuffer_motion_render(sah_ctx* ctx, const sah_scene_geometry* scene, const sah_view_data* view, const sah_gbuffer* out,
                              const sah_plane* motion_vectors, uint32_t* stats) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!geometry_ok(scene, true) || !view || !out || !motion_vectors)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "gbuffer_motion_render: bad scene, view or targets");
    const uint32_t W = out->depth.width, H = out->depth.height;
    if (W == 0 || H == 0 || W > kMaxExtent || H > kMaxExtent) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "gbuffer_motion_render: extent must be 1..%u", kMaxExtent);
    if (const char* name = bad_gbuffer_target(out, W, H))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "gbuffer_motion_render: target '%s' has the wrong format, extent or alignment", name);
    if (!motion_target_ok(motion_vectors, W, H))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "gbuffer_motion_render: 'motion_vectors' must be an R16G16_SFLOAT plane of the depth plane's extent, 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_raster));
    if (int rc = ensure_srgb_table(ctx); rc != SAH_OK) return rc;
    sah::RasterArgs a{};
    fill_scene(ctx, a, scene);
    fill_gbuffer(ctx, a, view, out);
    fill_motion(a, view, &out->depth, motion_vectors);
    return run(ctx, a, scene, sah::RasterPass::GBufferMotion, stats);
}

int sah_rsm_render(sah_ctx* ctx, const sah_scene_geometry* scene, const sah_sun_light_constants* sun, const sah_lpv_cascade_matrices* cascades,
                   uint32_t num_cascades, const sah_rsm_targets* rsm, uint32_t* stats) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!geometry_ok(scene, true) || !sun || !cascades || !rsm || num_cascades == 0 || num_cascades > 4)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rsm_render: bad scene, sun, cascades or targets");
    const uint32_t W = rsm->depth.width, H = rsm->depth.height;
    if (W == 0 || H == 0 || W > kMaxExtent || H > kMaxExtent) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "rsm_render: extent must be 1..%u", kMaxExtent);
    const struct { const sah_volume* v; uint32_t fmt; uint32_t bpp; const char* name; } targets[3] = {
        {&rsm->flux, SAH_FORMAT_R8G8B8A8_SRGB, 4, "flux"}, {&rsm->normals, SAH_FORMAT_R8G8B8A8_UNORM, 4, "normals"}, {&rsm->depth, SAH_FORMAT_D16_UNORM, 2, "depth"}};
    for (const auto& t : targets)
        if (!t.v->ptr || t.v->format != t.fmt || t.v->width != W || t.v->height != H || t.v->depth < num_cascades ||
            (uint64_t)t.v->row_pitch_bytes < (uint64_t)W * t.bpp || (uint64_t)t.v->slice_pitch_bytes < (uint64_t)t.v->row_pitch_bytes * H ||
            ((uintptr_t)t.v->ptr % t.bpp) || (t.v->row_pitch_bytes % t.bpp) || (t.v->slice_pitch_bytes % t.bpp))
            return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "rsm_render: target '%s' has the wrong format, extent, layers or alignment", t.name);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_raster));
    if (int rc = ensure_srgb_table(ctx); rc != SAH_OK) return rc;
    sah::RasterArgs a{};
    fill_scene(ctx, a, scene);
    a.num_views = num_cascades;
    for (uint32_t c = 0; c < num_cascades; c++) std::memcpy(a.clip_matrix[c], cascades[c].rsm_vp, 64);
    fill_extent(a, W, H);
    a.half_to_srgb8 = ctx->raster.half_to_srgb8;
    for (int k = 0; k < 3; k++) a.sun_direction[k] = sun->direction_and_tan_size[k];
    a.rsm_flux = varg(rsm->flux);
    a.rsm_normals = varg(rsm->normals);
    a.rsm_depth = varg(rsm->depth);
    return run(ctx, a, scene, sah::RasterPass::Rsm, stats);
}

int sah_motion_vectors_render(sah_ctx* ctx, const sah_scene_geometry* scene, const sah_view_data* view, const sah_plane* depth,
                              const sah_plane* motion_vectors, uint32_t* stats) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!geometry_ok(scene, false) || !view || !depth || !motion_vectors)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_vectors_render: bad scene, view or planes");
    const uint32_t W = depth->width, H = depth->height;
    if (W == 0 || H == 0 || W > kMaxExtent || H > kMaxExtent) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_vectors_render: extent must be 1..%u", kMaxExtent);
    if (!plane_ok(depth, SAH_FORMAT_D32_SFLOAT, SAH_FORMAT_D32_SFLOAT, W, H) || ((uintptr_t)depth->ptr % 4) || (depth->row_pitch_bytes % 4))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_vectors_render: 'depth' must be a D32_SFLOAT plane, 4-byte aligned, its pitch at least a row");
    // (r.MotionVectors.FullRes, a target of another extent than the depth buffer, is not supported: DESIGN.md §8)
    if (!motion_target_ok(motion_vectors, W, H))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_vectors_render: 'motion_vectors' must be an R16G16_SFLOAT plane of the depth plane's extent, 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_raster));
    sah::RasterArgs a{};
    fill_scene(ctx, a, scene);
    a.vertex_data = nullptr;  // positions, indices and primitives are all this pass reads
    a.materials = nullptr;
    a.textures = nullptr;
    a.material_textures = nullptr;
    a.num_textures = 0;
    a.num_views = 1;
    std::memcpy(a.view_matrix, view->view, 64);
    std::memcpy(a.clip_matrix[0], view->projection, 64);
    fill_extent(a, W, H);
    fill_motion(a, view, depth, motion_vectors);
    return run(ctx, a, scene, sah::RasterPass::Motion, stats);
}

// sah_translucent.h: the primitives of type TRANSLUCENT, set up as the G-buffer pass sets them up, peeled per tile in draw order, every fragment
// lit by the restatement of sah_lighting and blended into the lit image
int sah_translucent_render(sah_ctx* ctx, const sah_translucent_desc* desc) {
    SAH_RANGE();
    using namespace sah;
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!desc || !desc->lighting || !desc->scene) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "translucent_render: desc, its lighting desc and its scene are required");
    const sah_lighting_desc* d = desc->lighting;
    const sah_scene_geometry* scene = desc->scene;
    TranslucentShade t{};
    LightingCall call;
    SkyArgs sky;
    if (const int rc = lighting_targets(ctx, d, call, t.lighting); rc != SAH_OK) return rc;
    if (call.sun_mode == SAH_SHADOW_MODE_RT) return fail(ctx, SAH_ERR_UNSUPPORTED, "translucent_render: the ray-traced sun has no shadow mask for a translucent fragment (off and CSM are supported)");
    if (call.gi_kind == SAH_GI_CACHE || call.gi_kind == SAH_GI_RTGI)
        return fail(ctx, SAH_ERR_UNSUPPORTED, "translucent_render: GI kind %u does not light translucent fragments (none and LPV do)", call.gi_kind);
    if (d->lights && d->lights->count) return fail(ctx, SAH_ERR_UNSUPPORTED, "translucent_render: a light list does not light translucent fragments");
    if (const int rc = lighting_csm(ctx, d, call, t.csm); rc != SAH_OK) return rc;
    if (const int rc = lighting_gi_lpv(ctx, d, call, t.lpv); rc != SAH_OK) return rc;
    if (const int rc = lighting_sky(ctx, d, sky); rc != SAH_OK) return rc;  // (validated as sah_lighting validates it; a fragment is never sky)
    t.sun_mode = call.sun_mode;
    t.gi_kind = call.gi_kind;
    if (!geometry_ok(scene, true)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "translucent_render: bad scene");
    if (call.W > kMaxExtent || call.H > kMaxExtent) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "translucent_render: extent must be 1..%u", kMaxExtent);
    const sah_gbuffer& g = *d->gbuffer;
    if (((uintptr_t)g.depth.ptr % 4) || (g.depth.row_pitch_bytes % 4) || ((uintptr_t)d->lit->ptr % 8) || (d->lit->row_pitch_bytes % 8))
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "translucent_render: the depth plane must be 4-byte aligned and lit 8-byte aligned, pitches included");
    // lit is read and written in place: it must not share memory with a plane the call reads
    const auto span = [](const sah_plane& p, uint32_t bpp, uintptr_t& b, uintptr_t& e) {
        b = (uintptr_t)p.ptr;
        e = b + (uint64_t)(p.height - 1) * p.row_pitch_bytes + (uint64_t)p.width * bpp;
    };
    uintptr_t lb, le;
    span(*d->lit, 8, lb, le);
    const struct { const sah_plane* p; uint32_t bpp; } inputs[5] = {{&g.color, 4}, {&g.normals, 8}, {&g.data, 4}, {&g.emission, 4}, {&g.depth, 4}};
    for (const auto& in : inputs) {
        uintptr_t b, e;
        span(*in.p, in.bpp, b, e);
        if (lb < e && b < le) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "translucent_render: lit overlaps a plane of the G-buffer");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_raster));
    if (int rc = ensure_srgb_table(ctx); rc != SAH_OK) return rc;
    RasterArgs a{};
    fill_scene(ctx, a, scene);
    a.num_views = 1;
    a.shader_mip_bias = d->view->material_texture_mip_bias;
    std::memcpy(a.view_matrix, d->view->view, 64);
    std::memcpy(a.clip_matrix[0], d->view->projection, 64);
    fill_extent(a, call.W, call.H);
    a.half_to_srgb8 = ctx->raster.half_to_srgb8;
    return run(ctx, a, scene, RasterPass::Translucent, desc->stats, &t);
}

// Debug / test hook: how the last rasteriser call of the context (shadow, G-buffer, RSM, motion vectors or the fused pass) went through run() — recorded
// host side behind the synchronisation every attempt ends with; no device work.  All zero before the first call.
int sah_debug_raster_last_pass(sah_ctx* ctx, uint32_t out[4]) {
    if (!ctx || !out) return SAH_ERR_INVALID_ARGUMENT;
    std::memcpy(out, ctx->raster.last_pass, sizeof(ctx->raster.last_pass));
    return SAH_OK;
}

int sah_lpv_extract_vpls(sah_ctx* ctx, const sah_rsm_targets* rsm, const sah_lpv_cascade_matrices* cascades, uint32_t cascade_index,
                         float grid_cell_size, sah_packed_vpl* vpl_list, uint32_t* vpl_count) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!rsm || !cascades || !vpl_list || !vpl_count || cascade_index >= 4) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lpv_extract_vpls: null argument or cascade index");
    const uint32_t res = rsm->depth.width;
    if (res == 0 || (res % 2) || rsm->depth.height != res || rsm->flux.width != res || rsm->flux.height != res || rsm->normals.width != res ||
        rsm->normals.height != res || cascade_index >= rsm->depth.depth || cascade_index >= rsm->flux.depth || cascade_index >= rsm->normals.depth)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lpv_extract_vpls: the RSM layers must be square, of even size and cover the cascade");
    if (!rsm->flux.ptr || !rsm->normals.ptr || !rsm->depth.ptr || rsm->flux.format != SAH_FORMAT_R8G8B8A8_SRGB || rsm->normals.format != SAH_FORMAT_R8G8B8A8_UNORM ||
        rsm->depth.format != SAH_FORMAT_D16_UNORM)
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "lpv_extract_vpls: RSM formats are RGBA8_SRGB / RGBA8_UNORM / D16_UNORM");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_raster));
    const size_t invocations = (size_t)(res / 2) * (res / 2);
    if (int rc = ensure(ctx, S_VPL_CANDIDATES, invocations * (sizeof(sah_packed_vpl) + sizeof(uint32_t))); rc != SAH_OK) return rc;
    HIP_TRY(ctx, sah::launch_extract_vpls(varg(rsm->flux), varg(rsm->normals), varg(rsm->depth), cascades[cascade_index], cascade_index, grid_cell_size, ctx->luts,
                                          vpl_list, vpl_count, ctx->raster.buf[S_VPL_CANDIDATES].ptr, ctx->stream));
    return SAH_OK;
}

int sah_lpv_inject_vpls(sah_ctx* ctx, const sah_packed_vpl* vpl_list, const uint32_t* vpl_count, uint32_t capacity, const sah_lpv_cascade_matrices* cascades,
                        uint32_t cascade_index, uint32_t num_cascades, const sah_volume rgb[3]) {
    SAH_RANGE();
    if (ctx) ctx->lpv_copy.drop(ctx->cache_epoch);
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!vpl_list || !vpl_count || !cascades || !rgb || num_cascades == 0 || num_cascades > 4 || cascade_index >= num_cascades)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lpv_inject_vpls: null argument or cascade index");
    sah::VolumeArg v[3];
    for (int c = 0; c < 3; c++) {
        if (!rgb[c].ptr || rgb[c].format != SAH_FORMAT_R16G16B16A16_SFLOAT || rgb[c].width != rgb[0].width || rgb[c].height != rgb[0].height ||
            rgb[c].depth != rgb[0].depth || rgb[c].width == 0 || (uint64_t)rgb[c].row_pitch_bytes < (uint64_t)rgb[c].width * 8 ||
            (uint64_t)rgb[c].slice_pitch_bytes < (uint64_t)rgb[c].row_pitch_bytes * rgb[c].height || ((uintptr_t)rgb[c].ptr % 8) || (rgb[c].row_pitch_bytes % 8) ||
            (rgb[c].slice_pitch_bytes % 8) || (uint64_t)rgb[c].width * rgb[c].height * rgb[c].depth >= 0xffffffffull)
            return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "lpv_inject_vpls: the three volumes must be RGBA16F of one extent, 8-byte aligned");
        v[c] = varg(rgb[c]);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_raster));
    // cell index per light, then (16-byte aligned) the 12 blend sources of up to 4096 sorted lights (vpl.hip: k_inject_sorted)
    if (int rc = ensure(ctx, S_VPL_CELLS, ((size_t)capacity + 8) * sizeof(uint32_t) + (size_t)4096 * 12 * sizeof(float)); rc != SAH_OK) return rc;
    HIP_TRY(ctx, sah::launch_inject_vpls(vpl_list, vpl_count, capacity, cascades[cascade_index], cascade_index, num_cascades, v,
                                         (uint32_t*)ctx->raster.buf[S_VPL_CELLS].ptr, ctx->stream));
    return SAH_OK;
}

}  // extern "C"
