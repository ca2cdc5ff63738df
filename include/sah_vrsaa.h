/* sah_vrsaa.h — the two compute passes of the reference's own anti-aliasing mode, AntiAliasingType::VRSAA: contrast detection over the lit
 * frame and the shading-rate image made from it.
 *
 * SceneRenderer creates a VRSAA object when the mode is selected and renders at twice the output resolution
 * (RenderCore/render/scene_renderer.cpp:142-154); each frame it makes the shading-rate image from the LAST frame's contrast image before
 * the G-buffer pass (:357-361) and measures this frame's contrast after lighting (:476-481).  Host side:
 * RenderCore/render/phase/sampling_rate_calculator.cpp; shaders in RenderCore/shaders/vrsaa.  Same conventions as sah_hip.h (this header
 * includes it).  Parity unpinned: the reference ships no tests and no images of these passes; what its shaders leave open is fixed below
 * and marked "ABI-defined".
 *
 * Both calls run on the context's stream, do no host synchronisation, allocate nothing, leave their inputs and every cache and epoch of
 * the context untouched, and may be recorded under stream capture.  Consuming the shading-rate image (hardware VRS in the raster passes,
 * the reference's TODO at scene_renderer.cpp:479) is the caller's.
 */
#ifndef SAH_VRSAA_H
#define SAH_VRSAA_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_FORMAT_R8_UINT 13 /* VK_FORMAT_R8_UINT; accepted by the entries of this header only */

/* ShadingRateParams — sampling_rate_calculator.cpp:126-132, the uniform block `FrequencyInformation` of
 * generate_shading_rate_image.comp:8-15 (scalar layout): byte-identical, 92 bytes. */
typedef struct sah_shading_rate_params {
    uint32_t contrast_image_resolution[2];
    uint32_t shading_rate_image_resolution[2];
    uint32_t max_rate[2];
    uint32_t num_shading_rates;
    uint32_t rates[8][2];
} sah_shading_rate_params;

/* VRSAA::measure_aliasing — sampling_rate_calculator.cpp:55-76, contrast_detection.comp:15-68.
 *
 * Per pixel p of a W x H frame, in fp32 with every operator rounded on its own:
 * Taps       the nine taps (x, y) in [0, 2]^2, y outer and x inner (:37-38): s = p + (x, y) - 1, texcoord = float(s) / (W, H) (:39-40).
 * Sampler    the one VRSAA::VRSAA() creates (:17-23): NEAREST, CLAMP_TO_EDGE.  The texel is the one the library's NEAREST rule selects:
 *            index floor(texcoord * size) per axis, clamped to the image.  ABI-defined, and not clamp(s): fl(fl(s / n) * n) lies below s for
 *            some s (n = 97: s = 1, 2, 4, 7, 8, 13, ...), and the tap is then texel s - 1.
 * Luma       (r * 0.2126 + g * 0.7152) + b * 0.0722 of the sRGB-decoded texel (:13).  The reference binds gbuffer.color to `lit_scene`
 *            (scene_renderer.cpp:478), hence the format of `scene_color`.
 * Weights    sobel_x[x][y] = {1, 2, 1}[x] * {1, 0, -1}[y], sobel_y[x][y] = {1, 0, -1}[x] * {1, 2, 1}[y]: the shader indexes its column-major
 *            matrices [x][y] (:44-45), so the names are swapped relative to what they measure; the index is followed.
 * Sums       g.x += v * sobel_x[x][y], g.y += v * sobel_y[x][y] from +0 in tap order, once with v = luma and once with v = the raw depth
 *            value (:35-60).  Products with a zero weight are part of the sum: an infinite depth under one gives NaN.
 * Output     max(g_luma * 0.5, g_depth) per component (:62-67); max returns the other operand when one is NaN (the library's GLSL rule).
 *            The luma term is finite, so no NaN is ever stored.
 * Store      two halfs, round to nearest even, overflow to infinity.  The shader declares the image r16f while the view is
 *            R16G16_SFLOAT; ABI-defined: the view's format governs and both components are written — the only reading under which the
 *            second pass, which loads .xy, has defined input.
 *
 * scene_color: R8G8B8A8_SRGB, depth: D32_SFLOAT, contrast: R16G16_SFLOAT, all W x H, 4-byte aligned with pitches that are multiples of 4
 * and W * H < 2^32.  Rows [row_begin, row_end) of `contrast` are written ((0, 0) = all rows, as sah_copy_scene_rows); they read rows
 * [row_begin - 2, row_end + 1] of the inputs, clamped to the image.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer, a
 * zero extent, differing extents, a pitch smaller than a row, a misaligned plane, row_begin > row_end or row_end > H. */
int sah_vrsaa_measure_aliasing(sah_ctx* ctx, const sah_plane* scene_color, const sah_plane* depth, const sah_plane* contrast, uint32_t row_begin,
                               uint32_t row_end);

/* VRSAA::generate_shading_rate_image — sampling_rate_calculator.cpp:32-53, generate_shading_rate_image.comp:19-63.
 *
 * Per texel p of the shading-rate image:
 * d          max(1, uint(round(float(contrast_image_resolution.x) / float(shading_rate_image_resolution.x)))) (:26).  float(uvec2) takes
 *            .x, so the x ratio serves both axes.  round: ties to even — GLSL leaves the tie open; ABI-defined.
 * Maximum    m = max(m, |g * g|) per component from +0 over the texels (d * p.x + i, d * p.y + j), i, j < d, of `contrast` (:28-37); a texel
 *            outside the image reads 0; max ignores NaN.
 * Rate       a = min(1.25 * sqrt(m), 1); R = float(max(max_rate[0], max_rate[1])); optimal = a * 1 + (1 - a) * R (:39-44).
 * Search     cost_i = (float(rates[i][0]) - optimal.x)^2 + (float(rates[i][1]) - optimal.y)^2 for i < num_shading_rates, starting from
 *            1 + (2 * R) * R with index 0; a cost replaces the current one when strictly smaller, so the first of equal costs stays and
 *            num_shading_rates = 0 selects rates[0] (:46-57).
 * Code       (ry >> 1) | ((rx << 1) & 12) of the selected rate (:59-62), stored as one byte (ABI-defined: its low eight bits).
 *
 * contrast: R16G16_SFLOAT, 4-byte aligned, pitch a multiple of 4; shading_rate_image: R8_UINT of any extent >= 1 x 1 (the caller derives
 * it from its device's shading-rate texel size: ceil(resolution / texel size), sampling_rate_calculator.cpp:107-123).  params: host
 * memory, read during the call.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer, a
 * zero extent, a pitch smaller than a row, a misaligned contrast plane, params->contrast_image_resolution or
 * params->shading_rate_image_resolution differing from the planes' extents, num_shading_rates > 8, and (ABI-defined) extents at which
 * d * the shading-rate image's width or height reaches 2^31 or the contrast image has 2^32 texels or more. */
int sah_vrsaa_shading_rate_image(sah_ctx* ctx, const sah_plane* contrast, const sah_plane* shading_rate_image, const sah_shading_rate_params* params);

#ifdef __cplusplus
}
#endif

#endif /* SAH_VRSAA_H */
