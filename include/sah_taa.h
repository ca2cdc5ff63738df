/* sah_taa.h — temporal anti-aliasing: the consumer of the jitter (sah_view_data::jitter, previous_jitter) and of the motion vectors
 * (sah_motion_vectors.h, sah_gbuffer_motion.h).
 *
 * The reference's default anti-aliasing mode is an upscaler behind IUpscaler::evaluate(graph, view, gbuffer, color_in, color_out,
 * motion_vectors_in) (RenderCore/render/upscaling/upscaler.hpp:12-32, scene_renderer.cpp:483-497), and all three of its upscalers are
 * vendor binaries: there is no shader to follow.  This pass is builder-owned, like the point-light list: it sits where sah_copy_scene sits
 * (lit scene in, antialiased scene out, same format, same extent) and its arithmetic is fixed below ("ABI-defined"), restated in numpy by
 * tests/taa_ref.py and pinned bit for bit by tests/golden/taa_*.npz.  Parity unpinned: there is no reference output to compare with.  Same
 * conventions as sah_hip.h (this header includes it).
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing, leaves its inputs and every cache and epoch of
 * the context untouched, and may be recorded under stream capture.  A bicubic history tap and depth-based disocclusion tests are not part
 * of it.  Upscaling (render resolution != output resolution) is sah_taa_upscale's, in sah_taa_upscale.h.
 */
#ifndef SAH_TAA_H
#define SAH_TAA_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_TAA_HISTORY_INVALID 1u /* first frame / after a cut: `history` is not read (nor checked) and may be NULL */
#define SAH_TAA_HDR_WEIGHTS 2u     /* luminance-weighted blend (Weight, below); without it k = blend */

/* 24 bytes, host memory, read during the call.  jitter / previous_jitter: what sah_view_data carries for this frame, in pixels. */
typedef struct sah_taa_params {
    float blend; /* weight of the current frame, in (0, 1] */
    float jitter[2];
    float previous_jitter[2];
    uint32_t flags; /* SAH_TAA_* */
} sah_taa_params;

/* Per pixel (x, y) of a W x H frame, in fp32, every operator rounded on its own (no contraction) except the fma that is named.  All of it
 * is ABI-defined.
 * Current    c = rgb of lit[y][x], half -> float.
 * Bounds     the nine taps (dx, dy) in [-1, 1]^2 of `lit`, texel coordinates clamped to the image: lo, hi = per-channel min, max of the
 *            taps' rgb, taken from +inf and -inf.  min / max are the library's: a NaN operand is ignored, and -0 orders below +0 (so the
 *            result does not depend on the order of the taps).
 * Motion     the motion of the nearest surface of the neighbourhood: best = depth[y][x]; in tap order (dy outer, dx inner, the same clamped
 *            coordinates) a tap replaces the choice when its depth is strictly greater than best (reversed Z: greater is nearer; a NaN never
 *            replaces, and a NaN centre is never replaced).  mv = the two halfs of motion_vectors at the chosen texel.
 * Position   dj = previous_jitter - jitter (two fp32 subtractions on the host); q.x = ((float(x) + 0.5) + mv.x) + dj.x, likewise y.  The
 *            jitter shifts the raster by -jitter pixels, so a static camera's motion vector is jitter - previous_jitter, and mv + dj is the
 *            motion with the jitter taken out.
 * Validity   the history is valid for the pixel iff SAH_TAA_HISTORY_INVALID is clear and 0 <= q.x <= W and 0 <= q.y <= H (a NaN fails).
 * History    the library's bilinear rule at pixel coordinates: p = q - 0.5, i0 = floor(p), f = p - i0, indices i0 and i0 + 1 clamped to the
 *            edge, w00 = (1 - fx)(1 - fy), w10 = fx (1 - fy), w01 = (1 - fx) fy, w11 = fx fy, and per channel
 *            h = fma(w11, t11, fma(w01, t01, fma(w10, t10, fma(w00, t00, +0)))).  rgb only.  A non-finite channel of h makes the history
 *            invalid for the pixel.
 * Clamp      h' = min(max(h, lo), hi) per channel.
 * Weight     k = blend; with SAH_TAA_HDR_WEIGHTS: L(v) = max((v.r * 0.2126 + v.g * 0.7152) + v.b * 0.0722, 0), wc = blend / (1 + L(c)),
 *            wh = (1 - blend) / (1 + L(h')), k = wc / (wc + wh), IEEE divisions.
 * Blend      o = h' + (c - h') * k per channel: h' == c is a fixed point, bit for bit (but for a channel of -0, which leaves as +0:
 *            -0 + +0 = +0).
 * Store      rgb = o as halfs, round to nearest even, overflow to infinity.  Where the history is invalid or a channel of o is non-finite,
 *            the 16-bit patterns of lit's rgb are copied instead.  Alpha is always the 16 bits of lit's alpha.
 *
 * lit, history, out: R16G16B16A16_SFLOAT; depth: D32_SFLOAT, reversed Z as the G-buffer writes it; motion_vectors: R16G16_SFLOAT as
 * sah_motion_vectors_render writes it.  All W x H with W, H < 2^31 and W * H < 2^32, 4-byte aligned with pitches that are multiples of 4 (the rules of
 * sah_vrsaa_measure_aliasing); planes whose pointers and pitches are all multiples of 16 take the 16-byte path.  `history` is the
 * previous call's `out`: the caller ping-pongs two targets.
 *
 * Rows [row_begin, row_end) of `out` are written ((0, 0) = all rows); they read rows row_begin - 1 .. row_end of lit, depth and
 * motion_vectors, clamped to the image, and ANY row of `history`: under row sharding the history must be whole.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer
 * (`history` may be NULL only with SAH_TAA_HISTORY_INVALID), zero or differing extents, a pitch smaller than a row, a misaligned plane,
 * row_begin > row_end or row_end > H, blend outside (0, 1], a non-finite jitter, unknown flag bits, and the byte range of `out`
 * overlapping that of any input (the 3 x 3 reads make in-place unsafe). */
int sah_taa_resolve(sah_ctx* ctx, const sah_plane* lit, const sah_plane* depth, const sah_plane* motion_vectors, const sah_plane* history,
                    const sah_plane* out, const sah_taa_params* params, uint32_t row_begin, uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_TAA_H */
