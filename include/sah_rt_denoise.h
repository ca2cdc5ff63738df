/* sah_rt_denoise.h — temporal and edge-aware filter for the one-channel ray-traced planes: the AO plane of sah_rtao and the sun's mask of
 * sah_sun_shadow_mask (sah_hip.h).  Both are noise by construction — sah_rtao keeps the reference's quirk that every ray of a pixel reads
 * the same noise texel, so its plane is 0 or 1 per pixel — and the reference never shows them raw: its default anti-aliasing path is a
 * vendor ray-reconstruction upscaler, and the RTGI denoiser it carries is commented out.  There is no shader to follow.  This pass is
 * builder-owned, like sah_taa_resolve and sah_ssao: reprojected temporal accumulation with a disocclusion test, then an edge-stopping
 * a-trous filter.  Its arithmetic is fixed below ("ABI-defined"), restated in numpy by tests/rt_denoise_ref.py and pinned bit for bit by
 * tests/golden/rt_denoise_*.npz.  Parity unpinned: there is no reference output to compare with.  Same conventions as sah_hip.h (this
 * header includes it).
 *
 * NOT part of it: variance-guided or history-length-adaptive filter widths and RGB planes (ray_irradiance) — those are
 * sah_rtgi_denoise.h's — a previous-normals test, bicubic history, feeding the filtered value back into the history, sah_chain_*
 * integration, any change to sah_rtao or sah_sun_shadow_mask.
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing and asks no scratch of the caller (the filter's
 * iterations chain through LDS), leaves its inputs and every cache and epoch of the context untouched, may be recorded under stream
 * capture, and makes at most two launches.
 */
#ifndef SAH_RT_DENOISE_H
#define SAH_RT_DENOISE_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_RT_DENOISE_HISTORY_INVALID 1u /* first frame / after a cut: previous_depth, history and history_length are neither read nor checked and may be NULL */

/* 40 bytes, host memory, read during the call.  The defaults are design choices, not measurements. */
typedef struct sah_rt_denoise_params {
    float max_history;         /* cap of the sample count, in [1, 256]; default 32 */
    float depth_tolerance;     /* reprojection: relative difference of linear depth a history tap may have; finite and > 0; default 0.1 */
    float depth_sharpness;     /* filter: a neighbour whose relative depth difference reaches 1 / depth_sharpness has no weight; finite and >= 0; default 50 (sah_ssao's edge_sharpness) */
    uint32_t normal_squarings; /* filter: the normal weight is max(n_c . n_t, 0) ^ (2 ^ normal_squarings); 0..7; default 5 */
    uint32_t passes;           /* a-trous iterations, strides 1, 2, 4; 0..3; default 3 */
    float jitter[2];           /* what sah_view_data carries for this frame, in pixels */
    float previous_jitter[2];
    uint32_t flags;            /* SAH_RT_DENOISE_* */
} sah_rt_denoise_params;

/* Ten planes of one extent W x H.  in: this frame's; previous_depth, history, history_length: the last frame's depth and the last
 * call's accum_out and length_out (the caller ping-pongs them).  The history is never fed the filtered value. */
typedef struct sah_rt_denoise_desc {
    const sah_plane* noisy;          /* in  R32_SFLOAT: the output of sah_rtao or sah_sun_shadow_mask */
    const sah_plane* depth;          /* in  D32_SFLOAT, reversed Z as the G-buffer writes it */
    const sah_plane* normals;        /* in  R16G16B16A16_SFLOAT, world space, unnormalised (the G-buffer's) */
    const sah_plane* motion_vectors; /* in  R16G16_SFLOAT as sah_motion_vectors_render writes it */
    const sah_plane* previous_depth; /* in  D32_SFLOAT */
    const sah_plane* history;        /* in  R32_SFLOAT */
    const sah_plane* history_length; /* in  R16_SFLOAT */
    const sah_plane* accum_out;      /* out R32_SFLOAT: the temporally accumulated, spatially UNfiltered value */
    const sah_plane* length_out;     /* out R16_SFLOAT: its sample count */
    const sah_plane* denoised;       /* out R32_SFLOAT: the plane sah_lighting reads as `ao` or `shadow_mask` */
} sah_rt_denoise_desc;

/* Per pixel (x, y), in fp32, every operator rounded on its own (no fma anywhere), IEEE division and square root.  All of it is
 * ABI-defined.  Written out: max0(a) = a > 0 ? a : 0 (a NaN gives 0), min(a, b) = a < b ? a : b, finite(a) = |a| < inf.
 * View       The pass assumes the projection SceneView produces (sah_ssao.h, "View") and reads P00 = projection[0], P11 = projection[5],
 *            P20 = projection[8], P21 = projection[9], z_near, rows 0..2 of inverse_view (IV, column major) and row 2 of
 *            last_frame_view (L).  The host forms ipx = 1 / P00, ipy = 1 / P11, tx = 2 / float(W), ty = 2 / float(H) and
 *            dj = previous_jitter - jitter once.
 * Surface    d = depth[y][x]; !(d > 0) has no surface.  Otherwise z = z_near / d, P is sah_ssao's Position:
 *            P = ((z * (((float(x) + 0.5) * tx - 1) + P20)) * ipx, (z * (((float(y) + 0.5) * ty - 1) + P21)) * ipy, -z);
 *            n = the rgb halfs of normals[y][x] as floats, l = sqrt((n.x * n.x + n.y * n.y) + n.z * n.z), N = n / l (three divisions).  The
 *            pixel HAS A SURFACE iff d > 0 and every component of P and N is finite.  A pixel without one stores the 32 bits of
 *            noisy[y][x] to accum_out and to denoised, and length 0; nothing below applies to it, and no other pixel reads it.
 * Sample     c = noisy[y][x] where that is finite, else 1.0.
 * Reproject  mv = the two halfs of motion_vectors[y][x] (the pixel's own: no dilation); q.x = ((float(x) + 0.5) + mv.x) + dj.x, likewise y
 *            (sah_taa_resolve's "Position").  world_i = ((IV[i] * P.x + IV[4 + i] * P.y) + IV[8 + i] * P.z) + IV[12 + i] for i = 0, 1, 2;
 *            z_prev = -(((L[2] * world.x + L[6] * world.y) + L[10] * world.z) + L[14]): the linear depth last frame's camera saw this point
 *            at (the reference has no per-object previous transform, so this is exact for whatever the rasteriser drew; it is what keeps
 *            the history through a dolly).  tol = depth_tolerance * z_prev.
 *            The library's bilinear rule at p = q - 0.5: i0 = floor(p), f = p - i0, g = 1 - f, and the four taps in the order
 *            (i0.x, i0.y), (i0.x + 1, i0.y), (i0.x, i0.y + 1), (i0.x + 1, i0.y + 1) with weights g.x * g.y, f.x * g.y, g.x * f.y, f.x * f.y.
 *            A tap is VALID iff its weight is > 0, it lies inside the image (no clamping), pd = previous_depth there is > 0,
 *            |z_near / pd - z_prev| <= tol, hv = history there is finite, and hl = history_length there (half -> float) is finite and
 *            >= 1.  A tap of weight 0 or outside the image is not read.  From +0, over the valid taps in order: sw = sw + w,
 *            sh = sh + w * hv, sn = sn + w * hl.  (A static camera's q - 0.5 is the pixel: one tap of weight 1, and h below is its texel
 *            exactly.)
 *            The history is VALID for the pixel iff SAH_RT_DENOISE_HISTORY_INVALID is clear, 0 <= q.x <= W and 0 <= q.y <= H (a NaN
 *            fails), z_prev is finite and > 0, and sw > 0.
 * Accumulate with a valid history h = sh / sw, t = sn / sw + 1, n = min(t, max_history), a = c + (h - c) * (1 - 1 / n): h == c is a fixed
 *            point, bit for bit (but for -0, which leaves as +0).  Otherwise a = c, n = 1.  accum_out = a; length_out = n as a half, round
 *            to nearest even.
 * Filter     `passes` iterations i = 0, 1, 2 with stride s = 1, 2, 4; iteration i reads the plane v of iteration i - 1, iteration 0 reads
 *            a.  For the filter the unit normal is rounded: m_k = float(half(N_k)), to nearest even.  For a pixel with a surface:
 *            gc = depth_sharpness / z.  The nine taps (x + dx s, y + dy s), dy outer and dx inner, each from -1 to 1, with
 *            k = (1/4, 1/2, 1/4)[dx + 1] * (1/4, 1/2, 1/4)[dy + 1].  A tap outside the image or without a surface is left out.  The centre
 *            has w = 1/4.  Any other tap: dw = max0(1 - |z_t - z| * gc), e = max0((m.x * m_t.x + m.y * m_t.y) + m.z * m_t.z), then
 *            normal_squarings times e = e * e, and w = (k * dw) * e.  From +0 in tap order: W = W + w, D = D + w * (v_t - v).  The pixel's
 *            new value is v + D / W: a constant field is a fixed point, bit for bit.  denoised = the last iteration; passes == 0: a.
 *
 * All planes W x H with W, H < 2^31 and W * H < 2^32, 4-byte aligned with pitches that are multiples of 4 and at least a row (the rules
 * of sah_taa_resolve); when every plane's pointer and pitch is a multiple of 16 the temporal kernel takes the 16-byte path.
 *
 * Rows [row_begin, row_end) of `denoised` are written ((0, 0) = all rows), and a pixel's value does not depend on the row window.  With
 * r = 2^passes - 1, a non-empty band writes rows [max(row_begin - r, 0), min(row_end + r, H)) of accum_out and length_out and reads
 * the same rows of noisy, depth, normals and motion_vectors, and ANY row of previous_depth, history and history_length.  An empty band
 * writes and launches nothing.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer
 * (the three previous-frame planes may be NULL only with SAH_RT_DENOISE_HISTORY_INVALID), zero or differing extents, a pitch smaller
 * than a row, a misaligned plane, row_begin > row_end or row_end > H, max_history outside [1, 256], a depth_tolerance that is not finite
 * and > 0, a depth_sharpness that is not finite and >= 0, normal_squarings > 7, passes > 3, a non-finite jitter, unknown flag bits, a
 * NaN in any field of `view` the pass reads, a z_near that is not finite and positive, and the byte range of any output overlapping
 * that of any input or of another output. */
int sah_rt_denoise(sah_ctx* ctx, const sah_view_data* view, const sah_rt_denoise_desc* desc, const sah_rt_denoise_params* params,
                   uint32_t row_begin, uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_RT_DENOISE_H */
