/* sah_taa_upscale.h — temporal upscaling: sah_taa_resolve (sah_taa.h, which this header includes) with an output resolution above the
 * render resolution.  The frame is rendered, jittered, at w x h; the call reconstructs W x H from it, the motion vectors and the previous
 * W x H output.  Every pass of the library costs in proportion to the rendered pixels, so a frame rendered at 2560 x 1440 for a 3840 x 2160
 * output pays 1 / 2.25 of the raster, ray, lighting and GI work.
 *
 * It sits where the reference's IUpscaler::evaluate sits (RenderCore/render/upscaling/upscaler.hpp:12-32); the reference's upscalers are
 * vendor binaries, so the arithmetic is builder-owned like sah_taa_resolve's: fixed below ("ABI-defined"), restated in numpy by
 * tests/taa_upscale_ref.py and pinned bit for bit by tests/golden/taa_upscale_*.npz.  Parity unpinned.
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing, leaves its inputs and every cache and epoch of
 * the context untouched, and may be recorded under stream capture.  A bicubic or Lanczos history tap and depth-based disocclusion tests are
 * not part of it.
 */
#ifndef SAH_TAA_UPSCALE_H
#define SAH_TAA_UPSCALE_H

#include "sah_taa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 28 bytes, host memory, read during the call. */
typedef struct sah_taa_upscale_params {
    float blend;             /* weight of the current frame where the sample lies on the pixel's centre, in (0, 1] */
    float min_confidence;    /* floor of Confidence, in [0, 1] */
    float jitter[2];         /* this frame's, in RENDER pixels (sah_view_data::jitter) */
    float previous_jitter[2];
    uint32_t flags;          /* SAH_TAA_HISTORY_INVALID | SAH_TAA_HDR_WEIGHTS, the bits of sah_taa.h */
} sah_taa_upscale_params;

/* lit, depth, motion_vectors are w x h (the render resolution), history and out W x H (the output resolution), W >= w and H >= h; the two
 * ratios may differ.  Per pixel (X, Y) of `out`, in fp32, every operator rounded on its own (no contraction) except the fmas that are named.
 * All of it is ABI-defined.  The host forms, with IEEE operations, sx = float(w) / float(W), sy = float(h) / float(H), rx = float(W) /
 * float(w), ry = float(H) / float(h) and dj = previous_jitter - jitter.  Steps are given for x; y is likewise.
 * Sample     u.x = (float(X) + 0.5) * sx - jitter.x: the output pixel's centre in the jittered render raster (the jitter shifts the raster
 *            by -jitter pixels: sah_taa.h, Position).
 * Nearest    i = clamp(int(floor(u.x)), 0, w - 1), the float saturated to [-2^31, 2^31 - 128] before the conversion; j likewise.  u.x is
 *            monotone non-decreasing in X under fp32 rounding, and so is i.
 * Current    c = rgb of lit[j][i], half -> float.
 * Bounds, Motion
 *            exactly as sah_taa.h, for the 3 x 3 neighbourhood of texel (i, j) in the render planes: clamped taps, tap order, a NaN operand
 *            ignored, -0 below +0, a strictly nearer (greater) depth wins.  mv = the two halfs of motion_vectors at the chosen texel, in
 *            render pixels.
 * Position   in output pixels: q.x = (float(X) + 0.5) + (mv.x + dj.x) * rx.
 * Validity, History, Clamp
 *            as sah_taa.h over the W x H `history`: 0 <= q.x <= W and 0 <= q.y <= H, the bilinear rule with its fma chain and tap order, a
 *            non-finite channel of h makes the history invalid for the pixel, h' = min(max(h, lo), hi).
 * Confidence e.x = ((float(i) + 0.5) - u.x) * rx: how far, in output pixels, the sample lies from the pixel's centre.
 *            t = min(e.x * e.x + e.y * e.y, 1), g = 1 - t, conf = max(g * g, min_confidence), kb = blend * conf.
 * Weight     k = kb; with SAH_TAA_HDR_WEIGHTS wc = kb / (1 + L(c)), wh = (1 - kb) / (1 + L(h')), k = wc / (wc + wh), L as in sah_taa.h.
 * Blend      o = h' + (c - h') * k per channel.
 * Upsample   b = the bilinear rule applied to lit's rgb at u: p = u - 0.5, i0 = floor(p) (saturated as above), f = p - i0, taps i0 and
 *            i0 + 1 clamped to the render image, the four weights and the fma chain from +0 of History.  (floor(fl(u - 0.5)) is floor(u) - 1
 *            or floor(u) for every finite u, so the clamped taps always lie in the 3 x 3 neighbourhood of (i, j): no exceptions.)
 * Store      rgb = o as halfs (round to nearest even) where the history is valid and o is finite; otherwise b as halfs where its three
 *            channels are finite; otherwise the 16-bit patterns of lit[j][i]'s rgb.  Alpha is always the 16 bits of lit[j][i]'s alpha.
 *            With SAH_TAA_HISTORY_INVALID every pixel takes the "otherwise" chain, and `history` is neither read nor checked and may be NULL.
 *
 * lit, history, out: R16G16B16A16_SFLOAT; depth: D32_SFLOAT, reversed Z; motion_vectors: R16G16_SFLOAT in render pixels, as
 * sah_motion_vectors_render writes it.  Extents, alignment and the 16-byte path are sah_taa_resolve's: every width and height < 2^31,
 * w * h and W * H < 2^32, planes 4-byte aligned with pitches that are multiples of 4, and planes whose pointers and pitches are all multiples
 * of 16 take the 16-byte path.  `history` is the previous call's `out`: the caller ping-pongs two W x H targets.
 *
 * Rows [row_begin, row_end) of `out` are written ((0, 0) = all rows); they read rows j(row_begin) - 1 .. j(row_end - 1) + 1 of lit, depth
 * and motion_vectors, clamped to the image (j(Y) as under Nearest), and ANY row of `history`: under row sharding the history must be whole.
 *
 * Before anything is launched: the refusals of sah_taa_resolve (SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format;
 * SAH_ERR_INVALID_ARGUMENT for a NULL pointer — `history` may be NULL only with SAH_TAA_HISTORY_INVALID — a zero extent, a pitch smaller than
 * a row, a misaligned plane, row_begin > row_end or row_end > H, blend outside (0, 1], a non-finite jitter, unknown flag bits, the byte range
 * of `out` overlapping that of any input), and SAH_ERR_INVALID_ARGUMENT for w > W or h > H (downscaling), lit, depth and motion_vectors not
 * sharing one extent, history and out not sharing one extent, and min_confidence outside [0, 1] or NaN. */
int sah_taa_upscale(sah_ctx* ctx, const sah_plane* lit, const sah_plane* depth, const sah_plane* motion_vectors, const sah_plane* history,
                    const sah_plane* out, const sah_taa_upscale_params* params, uint32_t row_begin, uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_TAA_UPSCALE_H */
