// C ABI: camera motion blur (include/sah_motion_blur.h; kernels in motion_blur.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/sah_motion_blur.h"
#include "ctx.hpp"
#include "launch.hpp"

namespace {
// Nearest of the header for a row: the render row that output row Y sits on (the device's expression, operator by operator)
uint32_t nearest_row(uint32_t Y, float sy, float jy, uint32_t h) {
    volatile float centre = (float)Y + 0.5f;  // (volatile: each product and difference is rounded to fp32 on its own, whatever the host's flags)
    volatile float scaled = centre * sy;
    volatile float u = scaled - jy;
    const float f = std::fmin(std::fmax(std::floor(u), -2147483648.0f), 2147483520.0f);
    const int64_t j = (int64_t)f;
    return (uint32_t)(j < 0 ? 0 : j > (int64_t)h - 1 ? (int64_t)h - 1 : j);
}
}  // namespace

extern "C" int sah_motion_blur(sah_ctx* ctx, const sah_plane* scene, const sah_plane* depth, const sah_plane* motion_vectors, const sah_plane* tiles,
                               const sah_plane* out, const sah_motion_blur_params* params, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    static_assert(sizeof(sah_motion_blur_params) == 44, "sah_motion_blur_params is 44 bytes");
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!params) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: params is null");
    const sah_motion_blur_params& s = *params;
    if (s.flags & ~SAH_MOTION_BLUR_DITHER) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: an undefined flag bit is set");
    const PlaneSpec planes[5] = {{out, SAH_FORMAT_R16G16B16A16_SFLOAT, "out (R16G16B16A16_SFLOAT)"},
                                 {scene, SAH_FORMAT_R16G16B16A16_SFLOAT, "scene (R16G16B16A16_SFLOAT)"},
                                 {depth, SAH_FORMAT_D32_SFLOAT, "depth (D32_SFLOAT)"},
                                 {motion_vectors, SAH_FORMAT_R16G16_SFLOAT, "motion_vectors (R16G16_SFLOAT)"},
                                 {tiles, SAH_FORMAT_R16G16_SFLOAT, "tiles (R16G16_SFLOAT)"}};
    if (const int rc = check_planes(ctx, "motion_blur", planes, 5); rc != SAH_OK) return rc;
    const uint32_t W = out->width, H = out->height, w = depth->width, h = depth->height;
    if (scene->width != W || scene->height != H)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: scene and out must have one extent (the output resolution)");
    if (motion_vectors->width != w || motion_vectors->height != h)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: depth and motion_vectors must have one extent (the render resolution)");
    if (w > W || h > H) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: %u x %u to %u x %u is downscaling", w, h, W, H);
    if (texel_count_too_large(w, h) || texel_count_too_large(W, H)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: 2^32 texels or more");
    const uint32_t tiles_x = (w + SAH_MOTION_BLUR_TILE - 1) / SAH_MOTION_BLUR_TILE, tiles_y = (h + SAH_MOTION_BLUR_TILE - 1) / SAH_MOTION_BLUR_TILE;
    if (tiles->width != tiles_x || tiles->height != tiles_y)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: tiles must be ceil(w / 16) x ceil(h / 16) = %u x %u", tiles_x, tiles_y);
    if (!resolve_rows(&row_begin, &row_end, H)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: bad row range");
    for (const float v : {s.shutter, s.max_blur_pixels, s.min_velocity_pixels, s.depth_extent, s.z_near, s.jitter[0], s.jitter[1], s.previous_jitter[0],
                          s.previous_jitter[1]})
        if (std::isnan(v)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: a parameter is NaN");
    if (!(s.shutter > 0.0f && s.shutter <= 1.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: shutter must be in (0, 1]");
    if (!(s.max_blur_pixels > 0.0f && s.max_blur_pixels <= 32.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: max_blur_pixels must be in (0, 32]");
    if (!(std::isfinite(s.min_velocity_pixels) && s.min_velocity_pixels >= 0.0f))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: min_velocity_pixels must be finite and not negative");
    if (s.sample_count < 2 || s.sample_count > 32 || (s.sample_count & 1)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: sample_count must be even, 2..32");
    if (!(std::isfinite(s.depth_extent) && s.depth_extent > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: depth_extent must be finite and positive");
    if (!(std::isfinite(s.z_near) && s.z_near > 0.0f)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: z_near must be finite and positive");
    for (const float j : {s.jitter[0], s.jitter[1], s.previous_jitter[0], s.previous_jitter[1]})
        if (!std::isfinite(j)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: a jitter is not finite");
    for (int i = 1; i < 5; i++)
        if (overlaps(byte_range(out), byte_range(planes[i].p)))
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: out overlaps an input or tiles (the pass gathers along the motion: not in place)");
    for (int i = 1; i < 4; i++)
        if (overlaps(byte_range(tiles), byte_range(planes[i].p))) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "motion_blur: tiles overlaps an input");
    sah::MotionBlurArgs a{};
    a.scene = parg(scene), a.depth = parg(depth), a.mv = parg(motion_vectors), a.tiles = parg(tiles), a.out = parg(out);
    a.w = w, a.h = h, a.W = W, a.H = H, a.row_begin = row_begin, a.row_end = row_end;
    a.tiles_x = tiles_x, a.tiles_y = tiles_y;
    a.sx = (float)w / (float)W, a.sy = (float)h / (float)H;
    a.rx = (float)W / (float)w, a.ry = (float)H / (float)h;
    a.jx = s.jitter[0], a.jy = s.jitter[1];
    a.djx = s.previous_jitter[0] - s.jitter[0], a.djy = s.previous_jitter[1] - s.jitter[1];
    a.shutter = s.shutter, a.max_blur = s.max_blur_pixels, a.min_velocity = s.min_velocity_pixels, a.depth_extent = s.depth_extent;
    a.z_near = s.z_near, a.nf = (float)s.sample_count, a.sample_count = s.sample_count, a.flags = s.flags;
    // the tile rows the band's pixels select from: their own and one on either side
    const uint32_t t0 = nearest_row(row_begin, a.sy, a.jy, h) / SAH_MOTION_BLUR_TILE, t1 = nearest_row(row_end - 1, a.sy, a.jy, h) / SAH_MOTION_BLUR_TILE;
    a.tile_row_begin = t0 ? t0 - 1 : 0;
    a.tile_row_end = (t1 + 2 < tiles_y ? t1 + 2 : tiles_y);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_motion_blur(a, ctx->stream));
    return SAH_OK;
}
