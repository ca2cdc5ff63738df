// Every kernel launcher (sah::launch_*) and host helper that one translation unit of the library defines and another calls, declared once.
// Included by the callers (api*.cpp) AND by the defining files, so that the compiler checks each definition against the one declaration.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/sah_exposure.h"
#include "../../include/sah_hip.h"
#include "../../include/sah_mip_chain.h"
#include "../../include/sah_motion_blur.h"
#include "../../include/sah_rt_denoise.h"
#include "../../include/sah_rtgi_denoise.h"
#include "../../include/sah_sharpen.h"
#include "../../include/sah_ssao.h"
#include "../../include/sah_ssr.h"
#include "../../include/sah_sun_shafts.h"
#include "../../include/sah_taa.h"
#include "../../include/sah_taa_upscale.h"
#include "../../include/sah_vrs.h"
#include "../../include/sah_vrsaa.h"
#include "params.hpp"
#include "post_args.hpp"
#include "raster_args.hpp"
#include "rt_args.hpp"

struct sah_ctx;  // ctx.hpp

namespace sah {

// whether every plane's pointer and pitch are multiples of `align`: what lets a launcher pick its kernel's wide accesses
inline bool planes_aligned(std::initializer_list<const PlaneArg*> planes, uint32_t align) {
    bool ok = true;
    for (const PlaneArg* p : planes) ok = ok && ((uintptr_t)p->ptr % align) == 0 && (p->pitch % align) == 0;
    return ok;
}

// --- lighting.hip, lighting_tiled.hip
hipError_t launch_lighting(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const CacheArgs& cache, const RtgiArgs& rtgi,
                           const SkyArgs& sky, LightingFamily family, const FastArgs* fast, int sun_mode, int gi, int ppt, bool brute_force_lights,
                           hipStream_t st);
hipError_t launch_lighting_tiled(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const CacheArgs& cache, const RtgiArgs& rtgi,
                                 const SkyArgs& sky, int sun_mode, int gi, bool brute_force_lights, const FastArgs* fast, hipStream_t st);
bool lighting_fast_finishes_strays(bool sky_bound);  // whether that body of the fast kernel honours FastArgs::strays_inline (lighting.hip)
hipError_t launch_colx_table(const LightingArgs& a, const FastArgs& f, float* out, uint32_t stride, uint32_t row_stride, hipStream_t st);
hipError_t launch_probe_irr_unpack(const VolumeArg& src, uint8_t* dst, hipStream_t st);
hipError_t launch_probe_irr_unpack_probes(const VolumeArg& src, uint8_t* dst, const uint32_t* probes, uint32_t num_probes, hipStream_t st);

// --- post.hip, tonemap.hip, tonemap_tol.hip, sky_luts.hip
hipError_t launch_copy_scene(const PlaneArg& src, uint32_t sw, uint32_t sh, const PlaneArg& dst, uint32_t dw, uint32_t dh, uint32_t row_begin,
                             uint32_t row_end, hipStream_t st);
hipError_t launch_bloom_downsample(const PlaneArg& src, uint32_t sw, uint32_t sh, const PlaneArg& dst, uint32_t dw, uint32_t dh, uint32_t row_begin,
                                   uint32_t row_end, hipStream_t st);
bool launch_copy_bloom_mip0(const PlaneArg& lit, uint32_t lw, uint32_t lh, const PlaneArg& aa, uint32_t aw, uint32_t ah, const PlaneArg& mip0, uint32_t mw, uint32_t mh,
                            uint32_t mip_row_begin, uint32_t mip_row_end, uint32_t aa_row_begin, uint32_t aa_row_end, hipStream_t st, hipError_t* err);
bool launch_bloom_pair(const PlaneArg& s, uint32_t sw, uint32_t sh, const PlaneArg& a, uint32_t aw, uint32_t ah, const PlaneArg& b, uint32_t bw, uint32_t bh,
                       hipStream_t st, hipError_t* err);
hipError_t launch_fill_r32f(const PlaneArg& dst, uint32_t w, uint32_t h, float value, hipStream_t st);
hipError_t launch_tonemap(const TonemapArgs& t, hipStream_t st);
hipError_t launch_tonemap_tol(const TonemapArgs& t, hipStream_t st);
hipError_t launch_tonemap_axis_tables(const TonemapArgs& t, TmAxis* out, hipStream_t st);
hipError_t launch_sky_luts(const PlaneArg& transmittance, const PlaneArg& multiscattering, const PlaneArg& sky_view, const float light_vector[3], hipStream_t st);

// --- vrsaa.hip
hipError_t launch_vrsaa_contrast(const PlaneArg& color, const PlaneArg& depth, const PlaneArg& out, uint32_t w, uint32_t h, uint32_t row_begin,
                                 uint32_t row_end, const float* luts, hipStream_t st);
hipError_t launch_vrsaa_shading_rate(const PlaneArg& contrast, uint32_t cw, uint32_t ch, const PlaneArg& out, uint32_t sw, uint32_t sh, uint32_t d,
                                     const sah_shading_rate_params& params, hipStream_t st);

// --- lighting_vrs.hip, vrs_resolve.hip
struct VrsArgs {
    PlaneArg rate;                      // R8_UINT shading-rate image
    uint32_t texel_shift[2];            // log2 of the texel size, per axis
    float depth_tolerance;
    uint32_t vec4;                      // the depth and lit planes allow 16-byte accesses and the width is a multiple of 4
};
hipError_t launch_lighting_vrs(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const SkyArgs& sky, const VrsArgs& v, int sun_mode, int gi,
                               hipStream_t st);
hipError_t launch_vrsaa_resolve(const PlaneArg& lit, const PlaneArg& out, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_end, hipStream_t st);

// --- taa.hip
struct TaaArgs {
    PlaneArg lit, depth, mv, history, out;  // history: null without a history (the kernel then copies lit)
    uint32_t W, H, row_begin, row_end;
    float blend, djx, djy;                  // dj = previous_jitter - jitter
};
hipError_t launch_taa_resolve(const TaaArgs& a, bool history, bool hdr_weights, hipStream_t st);

// --- taa_upscale.hip
struct TaaUpscaleArgs {
    PlaneArg lit, depth, mv, history, out;  // lit, depth, mv: w x h; history (null without a history), out: W x H
    uint32_t w, h, W, H, row_begin, row_end;
    float blend, min_confidence, jx, jy, djx, djy;  // j = jitter, dj = previous_jitter - jitter
    float sx, sy, rx, ry;                           // fl(w / W), fl(h / H), fl(W / w), fl(H / h)
};
hipError_t launch_taa_upscale(const TaaUpscaleArgs& a, bool history, bool hdr_weights, hipStream_t st);

// --- ssao.hip
struct SsaoArgs {
    PlaneArg depth, normals, raw, out;  // raw: what the raw pass writes and the blur reads (scratch; ao_out itself without a blur)
    uint32_t W, H;
    uint32_t raw_begin, raw_end;        // rows of `raw` the raw pass writes: the band widened by the blur's reach, clipped to the image
    uint32_t row_begin, row_end;        // rows of `out`
    float m[9];                         // the 3 x 3 of view, column major: m[3 * column + row]
    float p20, p21, ipx, ipy, tx, ty;   // 1 / P00, 1 / P11, 2 / W, 2 / H
    float sx, rs, z_near;               // (0.5 W) P00, radius * sx
    float max_radius_pixels, threshold, shadow_multiplier, shadow_clamp, fade_to, fade_span, edge_sharpness;
};
hipError_t launch_ssao(const SsaoArgs& a, uint32_t blur_passes, hipStream_t st);

// --- ssr.hip
struct SsrArgs {
    PlaneArg color, normals, data, depth, source, lit, out;
    uint32_t W, H;
    uint32_t row_begin, row_end;        // rows of `out`
    uint32_t tiles_x;                   // set by the launcher
    float m[9];                         // the 3 x 3 of view, column major: m[3 * column + row]
    float p00, p11, p20, p21, ipx, ipy, tx, ty, hw, hh;  // 1 / P00, 1 / P11, 2 / W, 2 / H, 0.5 W, 0.5 H
    float z_near;
    float max_distance, thickness, stride, max_roughness, edge_fade, intensity;
    uint32_t max_steps, refine_steps, flags;
    const float* luts;                  // the context's 512 floats: sRGB -> linear, UNORM8 -> float
};
hipError_t launch_ssr(const SsrArgs& a, hipStream_t st);

// --- motion_blur.hip
struct MotionBlurArgs {
    PlaneArg scene, depth, mv, tiles, out;  // scene, out: W x H; depth, mv: w x h; tiles: tiles_x x tiles_y
    uint32_t w, h, W, H;
    uint32_t row_begin, row_end;            // rows of `out`
    uint32_t tiles_x, tiles_y;              // ceil(w / 16), ceil(h / 16)
    uint32_t tile_row_begin, tile_row_end;  // rows of `tiles` the band needs: its own tile rows and one on either side
    uint32_t groups_x;                      // set by the launcher
    float sx, sy, rx, ry;                   // fl(w / W), fl(h / H), fl(W / w), fl(H / h)
    float jx, jy, djx, djy;                 // j = jitter, dj = previous_jitter - jitter
    float shutter, max_blur, min_velocity, depth_extent, z_near, nf;  // nf = float(sample_count)
    uint32_t sample_count, flags;
};
hipError_t launch_motion_blur(const MotionBlurArgs& a, hipStream_t st);

// --- sun_shafts.hip
struct SunShaftsArgs {
    PlaneArg depth, lit, march, out;        // depth, lit, out: w x h; march: mw x mh
    CsmArgs csm;                            // Lighting's block: the map, the splits and the biased matrices (shadowmap.ptr null: all lit)
    uint32_t w, h, mw, mh;
    uint32_t row_begin, row_end;            // rows of `out`
    uint32_t march_row_begin, march_row_end;  // rows of `march` the band writes
    uint32_t groups_x;                      // set by the launcher
    uint32_t downscale, num_steps, num_cascades, dither_offset, flags;
    float wf, hf;                           // float(w), float(h)
    float inv_proj[16], inv_view[16];
    float a[4][3];                          // a_c: the camera in cascade c's divided coordinates
    float lv[3], sun_color[3], albedo[3], ambient[3];
    float step_length, d_min, z_near, depth_bias, depth_sharpness;
    float g1, g2, g3;                       // 1 + g g, 1 - g g, 2 g
    float D[SAH_SUN_SHAFTS_MAX_STEPS];      // the energy a step removes
};
hipError_t launch_sun_shafts(const SunShaftsArgs& a, hipStream_t st);

// --- exposure.hip
struct ExposureArgs {
    PlaneArg scene, out;              // out: exposed_out of the fused form / out of apply; unused by the metering alone
    uint32_t W, H;
    uint32_t row_begin, row_end;      // apply: rows of `out`
    uint32_t tiles_x, tiles;          // set by the launchers
    uint32_t* work;                   // SAH_EXPOSURE_WORK_BYTES: 256 bins, then the ticket word
    const sah_exposure_state* state_in;  // null without a history (meter); the state apply multiplies by
    sah_exposure_state* state_out;
    float key, low_fraction, high_fraction, min_exposure, max_exposure, adaptation;
    bool history;                     // SAH_EXPOSURE_HISTORY_INVALID is clear
};
hipError_t launch_exposure_meter(const ExposureArgs& a, bool apply, uint32_t max_workgroups, hipStream_t st);
hipError_t launch_exposure_apply(const ExposureArgs& a, hipStream_t st);

// --- sharpen.hip
struct SharpenArgs {
    PlaneArg scene, out;
    uint32_t W, H;
    uint32_t row_begin, row_end;         // rows of `out`
    uint32_t tiles_x;                    // set by the launcher
    const sah_exposure_state* exposure;  // device; null: k = pre_scale
    float sharpness, pre_scale;
};
hipError_t launch_sharpen(const SharpenArgs& a, bool denoise, hipStream_t st);

// --- rt_denoise.hip
struct RtDenoiseArgs {
    PlaneArg noisy, depth, normals, mv, prev_depth, history, hist_len, accum, length, out;
    uint32_t W, H;
    uint32_t acc_begin, acc_end;      // rows of `accum` and `length` the temporal kernel writes: the band widened by the filter's reach, clipped to the image
    uint32_t row_begin, row_end;      // rows of `out`
    float iv[12];                     // rows 0..2 of inverse_view, column major: iv[3 * column + row]
    float l2[4];                      // row 2 of last_frame_view
    float p20, p21, ipx, ipy, tx, ty;  // 1 / P00, 1 / P11, 2 / W, 2 / H
    float z_near, djx, djy;           // previous_jitter - jitter
    float max_history, depth_tolerance, depth_sharpness;
    uint32_t normal_squarings;
};
hipError_t launch_rt_denoise(const RtDenoiseArgs& a, uint32_t passes, bool history, hipStream_t st);

// --- rtgi_denoise.hip
struct RtgiDenoiseArgs {
    PlaneArg rays, irr, depth, normals, mv, prev_depth, history, hist_mom, accum, moments, out_rays, out_irr;
    uint32_t W, H;
    uint32_t acc_begin, acc_end;      // rows of `accum` and `moments` the temporal kernel writes: the band widened by the filter's reach, clipped to the image
    uint32_t row_begin, row_end;      // rows of `out_rays` and `out_irr`
    float iv[12];                     // rows 0..2 of inverse_view, column major: iv[3 * column + row]
    float l2[4];                      // row 2 of last_frame_view
    float p20, p21, ipx, ipy, tx, ty;  // 1 / P00, 1 / P11, 2 / W, 2 / H
    float z_near, djx, djy;           // previous_jitter - jitter
    float max_history, min_history, depth_tolerance, depth_sharpness, luminance_sigma, luminance_floor;
    uint32_t normal_squarings;
};
hipError_t launch_rtgi_denoise(const RtgiDenoiseArgs& a, uint32_t passes, bool history, hipStream_t st);

// --- mip_chain.hip
struct MipChainArgs {
    PlaneArg src;
    uint32_t src_w, src_h;
    float inv_w, inv_h;                                   // fl(1 / extent) of the source
    PlaneArg slot[SAH_MIP_CHAIN_MAX_LEVELS];              // imgDst[12]: level i, or level 1 from num_dst_levels on
    uint32_t slot_w[SAH_MIP_CHAIN_MAX_LEVELS], slot_h[SAH_MIP_CHAIN_MAX_LEVELS];  // what bounds a store to slot i: the extent level i has or would have
    uint32_t mips, num_workgroups;
    uint32_t* counter;
};
enum MipChainKind : int { kMipChainR32Min = 0, kMipChainR16 = 1, kMipChainRGBA16 = 2, kMipChainR11G11B10 = 3 };
hipError_t launch_mip_chain(const MipChainArgs& a, MipChainKind kind, hipStream_t st);

// --- lpv.hip, lpv_gv.hip, vpl.hip
hipError_t launch_lpv_clear(const VolumeArg* vols, int n, uint32_t num_cascades, hipStream_t st);
hipError_t launch_lpv_build_tables(hipStream_t st, bool* hot_structure);
hipError_t launch_lpv_propagate(const VolumeArg src[3], const VolumeArg dst[3], uint32_t num_cascades, const LpvPackEmit* emit, bool hot, hipStream_t st,
                                const LpvGvStep* gv = nullptr);
hipError_t launch_lpv_gv_factors(const VolumeArg& gv, void* factors, uint32_t num_cascades, hipStream_t st);
hipError_t launch_gv_inject_rsm(const VolumeArg& normals, const VolumeArg& depth, const sah_lpv_cascade_matrices* cascades, uint32_t first_cascade,
                                uint32_t cascade_count, uint32_t num_cascades, const VolumeArg& gv, uint32_t* keys, hipStream_t st);
hipError_t launch_gv_inject_scene(const PlaneArg& depth, const PlaneArg& normals, uint32_t width, uint32_t height, const sah_view_data& view,
                                  const sah_lpv_cascade_matrices* cascades, uint32_t num_cascades, const VolumeArg& gv, uint32_t* keys, hipStream_t st);
hipError_t launch_extract_vpls(const VolumeArg& flux, const VolumeArg& normals, const VolumeArg& depth, const sah_lpv_cascade_matrices& c, uint32_t cascade,
                               float grid_cell_size, const float* luts, sah_packed_vpl* list, uint32_t* count, void* scratch, hipStream_t st);
hipError_t launch_inject_vpls(const sah_packed_vpl* list, const uint32_t* count, uint32_t capacity, const sah_lpv_cascade_matrices& c, uint32_t cascade,
                              uint32_t num_cascades, const VolumeArg rgb[3], uint32_t* cells_scratch, hipStream_t st);

// --- probes.hip
hipError_t launch_probe_copy(const ProbeAtlasArgs& src, const ProbeAtlasArgs& dst, const float movement[4][3], hipStream_t st);
hipError_t launch_probe_update(const ProbeAtlasArgs& atl, const VolumeArg& trace, const uint32_t* probes, uint32_t num_probes, uint32_t* slots,
                               hipStream_t st);

// --- raster_setup.hip, raster_tiles.hip (the pass is a.pass)
hipError_t launch_raster_setup(const RasterArgs& a, hipStream_t st);
void launch_raster_fill_bins(const RasterArgs& a, hipStream_t st);  // raster_setup.hip's k_bin<fill>, first kernel of launch_raster_tiles
hipError_t launch_raster_tiles(const RasterArgs& a, hipStream_t st);
// the tile stage of RasterPass::Translucent (sah_translucent.h): what sah_lighting's stages made of the frame's Lighting descriptor, which
// lights every fragment; `lighting` also names the lit image, the depth plane tested against and the row range
struct TranslucentShade {
    LightingArgs lighting;
    CsmArgs csm;
    LpvArgs lpv;
    uint32_t sun_mode, gi_kind;  // off or CSM; none or LPV
};
hipError_t launch_translucent_tiles(const RasterArgs& a, const TranslucentShade& t, hipStream_t st);

// --- rt.hip
hipError_t launch_rt_scan(const sah_primitive* prims, uint32_t n, uint32_t* tri_base, RtBuildState* st, hipStream_t s);
hipError_t launch_rt_world(const RtScene& sc, const uint32_t* tri_base, uint32_t total, RtTriangle* out, RtBuildState* st, hipStream_t s);
hipError_t launch_rt_sort(const RtTriangle* tris, const RtBuildState* st, unsigned long long* keys, uint32_t padded, hipStream_t s);
hipError_t launch_rt_nodes(const RtTriangle* unsorted, const unsigned long long* keys, RtTriangle* sorted, RtNodeGroup* nodes, const RtBvh& bvh, hipStream_t s);
hipError_t launch_rtao(const RtaoArgs& a, const RtBvh& bvh, const RtScene& sc, hipStream_t s);
hipError_t launch_sun_shadow_mask(const ShadowMaskArgs& a, const RtBvh& bvh, const RtScene& sc, hipStream_t s);
hipError_t launch_noise_dirs(const PlaneArg& noise, const float* luts, float* out, hipStream_t s);
hipError_t launch_probe_trace(const ProbeTraceArgs& a, const RtBvh& bvh, const RtScene& sc, hipStream_t s);
hipError_t launch_rtgi_trace(const RtgiTraceArgs& a, const RtBvh& bvh, const RtScene& sc, hipStream_t s);

// --- rt_refit.hip
hipError_t launch_rt_refit(const RtScene& sc, const RtBvh& bvh, RtTriangle* tris, RtNodeGroup* nodes, RtBuildState* st, uint32_t* stats, hipStream_t s);

// --- ipc.hip (direct exchange)
struct IpcPeers {
    uint32_t* slot[SAH_IPC_MAX_WORLD];  // where to store (signal) / what to poll (wait); null: skipped
};
struct IpcCopies {
    uint8_t* dst[SAH_IPC_MAX_WORLD];  // the own slot inside every peer's buffer; null: skipped
};
hipError_t launch_ipc_signal(const IpcPeers& peers, uint32_t value, const uint32_t* abort, hipStream_t st);
hipError_t launch_ipc_wait(const IpcPeers& own, uint32_t value, uint32_t* abort, uint32_t* timed_out, const IpcPeers& notes, hipStream_t st);
hipError_t launch_ipc_copy(const IpcCopies& c, int world, const uint8_t* src, uint64_t bytes, const uint32_t* abort, const uint32_t* gave_up, hipStream_t st);

}  // namespace sah

// --- api_ipc.cpp: the direct exchange as the other entry points use it
int sah_ipc_find(const sah_ctx* ctx, const void* ptr, uint64_t bytes);
int sah_ipc_gather(sah_ctx* ctx, uint32_t id, uint8_t* buffer, uint64_t bytes_per_rank, bool reversed, hipStream_t st);
bool sah_ipc_timed_out(const sah_ctx* ctx);
