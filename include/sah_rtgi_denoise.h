/* sah_rtgi_denoise.h — temporal accumulation and a variance-guided, edge-aware filter for the two RGB planes of sah_rtgi_trace
 * (sah_hip.h): ray_buffer (direction, distance) and ray_irradiance, one GI ray per pixel.  At the reference's default
 * (r.GI.Reconstruction.NumSamples = 0) the RTGI mode of sah_lighting lights from that one-sample estimate; the reference expects a
 * vendor ray-reconstruction upscaler to clean it, and the 3 x 3 average in its overlay is commented out.  There is no shader to follow.
 * This pass is builder-owned, like sah_rt_denoise (whose rules it cites by name; this header includes that one): its arithmetic is fixed
 * below ("ABI-defined"), restated in numpy by tests/rtgi_denoise_ref.py and pinned bit for bit by tests/golden/rtgi_denoise_*.npz.
 * Parity unpinned: there is no reference output to compare with.
 *
 * Design decision — the quantity that is filtered.  The overlay computes brdf(surface, dir, V) * irr * clamp(dir . N) per ray; a random
 * direction per pixel per frame cannot be averaged.  The pass accumulates the cosine-weighted irradiance E = irr * clamp(dir . N), the
 * quantity a diffuse surface integrates, and hands back a PAIR of planes the unchanged overlay consumes: a ray buffer whose direction
 * is the surface normal, and an irradiance plane holding the filtered E'.  The overlay then evaluates brdf(surface, N, V) * E' *
 * clamp(N . N): exact for a Lambert surface, and the approximation the reference's own irradiance-cache overlay makes
 * (gi/cache/overlay.frag.slang:93-98, L = N).
 *
 * Design decision — what guides the filter.  Irradiance has edges (contact shadows, colour bleeding) that are in neither depth nor
 * normals.  Besides the depth and normal weights of sah_rt_denoise a tap carries a luminance weight whose width is the local standard
 * deviation of the accumulated luminance (from two accumulated moments); it is switched off for a centre pixel with fewer than
 * min_history samples, whose variance estimate is worthless.
 *
 * NOT part of it: a previous-normals test, bicubic history, feeding the filtered value back into the history, specular or
 * direction-dependent reconstruction, sah_chain_* integration, any change to sah_rtgi_trace, sah_lighting or sah_rt_denoise.
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing and asks no scratch of the caller (the filter's
 * iterations chain through LDS), leaves its inputs and every cache and epoch of the context untouched, may be recorded under stream
 * capture, and makes at most two launches, one after the other.
 */
#ifndef SAH_RTGI_DENOISE_H
#define SAH_RTGI_DENOISE_H

#include "sah_rt_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_RTGI_DENOISE_HISTORY_INVALID 1u /* first frame / after a cut: previous_depth, history and history_moments are neither read nor checked and may be NULL */

#define SAH_FORMAT_R32G32_SFLOAT 103       /* VK_FORMAT_R32G32_SFLOAT; accepted by the entry of this header only */
#define SAH_FORMAT_R32G32B32A32_SFLOAT 109 /* VK_FORMAT_R32G32B32A32_SFLOAT; likewise */

/* 52 bytes, host memory, read during the call.  The defaults are design choices, not measurements. */
typedef struct sah_rtgi_denoise_params {
    float max_history;         /* cap of the sample count, in [1, 256]; default 32 */
    float min_history;         /* a centre pixel with fewer samples filters without the luminance term, in [1, 256]; default 4 */
    float depth_tolerance;     /* reprojection: relative difference of linear depth a history tap may have; finite and > 0; default 0.1 */
    float depth_sharpness;     /* filter: a neighbour whose relative depth difference reaches 1 / depth_sharpness has no weight; finite and >= 0; default 50 */
    uint32_t normal_squarings; /* filter: the normal weight is max(n_c . n_t, 0) ^ (2 ^ normal_squarings); 0..7; default 5 */
    uint32_t passes;           /* a-trous iterations, strides 1, 2, 4; 0..3; default 3 */
    float luminance_sigma;     /* filter: a tap whose luminance differs by luminance_sigma standard deviations has no weight; finite and >= 0; 0 leaves the term out of every weight; default 4 */
    float luminance_floor;     /* added to that width; finite and > 0; default 1e-6 */
    float jitter[2];           /* what sah_view_data carries for this frame, in pixels */
    float previous_jitter[2];
    uint32_t flags;            /* SAH_RTGI_DENOISE_* */
} sah_rtgi_denoise_params;

/* Twelve planes of one extent W x H.  in: this frame's; previous_depth, history, history_moments: the last frame's depth and the last
 * call's accum_out and moments_out (the caller ping-pongs them).  The history is never fed the filtered value.  The history is fp32 on
 * purpose: the irradiance is scaled by 0.0031415927 at the trace, a running mean of mostly-zero samples sits near the half subnormals,
 * and the variance is a difference of squares. */
typedef struct sah_rtgi_denoise_desc {
    const sah_plane* ray_buffer;          /* in  R16G16B16A16_SFLOAT: direction, distance (sah_rtgi_trace) */
    const sah_plane* ray_irradiance;      /* in  R16G16B16A16_SFLOAT */
    const sah_plane* depth;               /* in  D32_SFLOAT, reversed Z as the G-buffer writes it */
    const sah_plane* normals;             /* in  R16G16B16A16_SFLOAT, world space, unnormalised (the G-buffer's) */
    const sah_plane* motion_vectors;      /* in  R16G16_SFLOAT as sah_motion_vectors_render writes it */
    const sah_plane* previous_depth;      /* in  D32_SFLOAT */
    const sah_plane* history;             /* in  R32G32B32A32_SFLOAT: rgb = accumulated E, a = sample count */
    const sah_plane* history_moments;     /* in  R32G32_SFLOAT: accumulated luminance and luminance squared */
    const sah_plane* accum_out;           /* out R32G32B32A32_SFLOAT: temporally accumulated, spatially UNfiltered */
    const sah_plane* moments_out;         /* out R32G32_SFLOAT */
    const sah_plane* denoised_ray_buffer; /* out R16G16B16A16_SFLOAT: what sah_lighting reads as gi.ray_buffer */
    const sah_plane* denoised_irradiance; /* out R16G16B16A16_SFLOAT: what sah_lighting reads as gi.ray_irradiance */
} sah_rtgi_denoise_desc;

/* Per pixel (x, y), in fp32, every operator rounded on its own (no fma anywhere), IEEE division and square root.  All of it is
 * ABI-defined.  max0, min and finite are those of sah_rt_denoise.h; clamp01(a) = a > 0 ? (a < 1 ? a : 1) : 0 (a NaN gives 0);
 * lum(c) = (0.2126 * c.r + 0.7152 * c.g) + 0.0722 * c.b.
 * View       as sah_rt_denoise.h.
 * Surface    as sah_rt_denoise.h: z, P, the fp32 unit normal N, and whether the pixel HAS A SURFACE.  A pixel without one stores the 64
 *            bits of ray_buffer[y][x] to denoised_ray_buffer and those of ray_irradiance[y][x] to denoised_irradiance, and zeros (+0)
 *            to accum_out and moments_out; nothing below applies to it, and no other pixel reads it.
 * Sample     dir = the rgb halfs of ray_buffer[y][x] as floats, irr = those of ray_irradiance[y][x];
 *            cs = clamp01((dir.x * N.x + dir.y * N.y) + dir.z * N.z); c.ch = irr.ch * cs, and a component that is not finite becomes +0.
 *            l = lum(c).
 * Reproject  as sah_rt_denoise.h: the pixel's own motion vector, z_prev from last_frame_view, tol, the four bilinear taps in that
 *            order, no clamping.  A tap is VALID iff its weight is > 0, it lies inside the image, pd = previous_depth there is > 0,
 *            |z_near / pd - z_prev| <= tol, hn = history.a there is finite and >= 1, and history.rgb and both of history_moments there
 *            are finite.  A tap of weight 0 or outside the image is not read.  From +0, over the valid taps in order: sw = sw + w,
 *            sn = sn + w * hn, and s_x = s_x + w * h_x for the five accumulated values x (history r, g, b, moments 0, 1).  The
 *            history is VALID for the pixel under the same conditions as there (with SAH_RTGI_DENOISE_HISTORY_INVALID).
 * Accumulate with a valid history n = min(sn / sw + 1, max_history), k = 1 - 1 / n, and each x of (c.r, c.g, c.b, l, l * l) becomes
 *            x + (s_x / sw - x) * k.  Otherwise the five values are themselves and n = 1.  accum_out = (r, g, b, n), moments_out =
 *            (m1, m2).  The filter's variance input is var = max0(m2 - m1 * m1).
 * Filter     `passes` iterations i = 0, 1, 2 with stride s = 1, 2, 4 over the pair (v: rgb, var); iteration 0 reads the accumulated
 *            pair, iteration i that of iteration i - 1.  The unit normal is rounded to half as in sah_rt_denoise.h (m).  For a
 *            centre pixel with a surface: lc = lum(v).
 *            g: over the nine STRIDE-1 neighbours (x + dx, y + dy), dy outer and dx inner, the centre included, that lie inside the
 *            image and have a surface, with k = (1/4, 1/2, 1/4)[dx + 1] * (1/4, 1/2, 1/4)[dy + 1]: from +0, gs = gs + k * var_t,
 *            ks = ks + k; g = gs / ks.  den = luminance_sigma * sqrt(g) + luminance_floor.
 *            The nine taps (x + dx s, y + dy s) with k, gc, dw and e exactly as in sah_rt_denoise.h; lw = max0(1 - |lum(v_t) - lc| / den),
 *            and lw = 1 when luminance_sigma == 0 or the CENTRE's sample count n (accum_out.a) < min_history.  w = ((k * dw) * e) * lw;
 *            the centre has w = 1/4.  A tap outside the image or without a surface is left out.  From +0 in tap order, the centre
 *            in its place: Ws = Ws + w, D.ch = D.ch + w * (v_t.ch - v.ch) per channel, Q = Q + (w * w) * var_t.
 *            New v.ch = v.ch + D.ch / Ws; new var = Q / (Ws * Ws).  A constant field is a fixed point, bit for bit.
 * Output     v' = the last iteration's v (passes == 0: the accumulated rgb).  denoised_ray_buffer = (half(N.x), half(N.y), half(N.z),
 *            the 16 bits of the input's distance); denoised_irradiance = (half(v'.r), half(v'.g), half(v'.b), +0), round to nearest
 *            even.
 *
 * All planes W x H with W, H < 2^31 and W * H < 2^32, 4-byte aligned with pitches that are multiples of 4 and at least a row (the rules
 * of sah_taa_resolve); when every plane's pointer and pitch is a multiple of 16 the temporal kernel takes the 16-byte path.
 *
 * Rows [row_begin, row_end) of the two denoised planes are written ((0, 0) = all rows), and a pixel's value does not depend on the row
 * window.  With r = 2^passes - 1, a non-empty band writes rows [max(row_begin - r, 0), min(row_end + r, H)) of accum_out and
 * moments_out and reads the same rows of the five planes of this frame, and ANY row of previous_depth, history and history_moments.
 * An empty band writes and launches nothing.
 *
 * Before anything is launched, with the status codes and rules of sah_rt_denoise: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another
 * format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer (the three previous-frame planes may be NULL only with
 * SAH_RTGI_DENOISE_HISTORY_INVALID), zero or differing extents, a pitch smaller than a row, a misaligned plane, row_begin > row_end or
 * row_end > H, max_history or min_history outside [1, 256], a depth_tolerance that is not finite and > 0, a depth_sharpness or
 * luminance_sigma that is not finite and >= 0, a luminance_floor that is not finite and > 0, normal_squarings > 7, passes > 3, a
 * non-finite jitter, unknown flag bits, a NaN in any field of `view` the pass reads, a z_near that is not finite and positive, and the
 * byte range of any output overlapping that of any input or of another output. */
int sah_rtgi_denoise(sah_ctx* ctx, const sah_view_data* view, const sah_rtgi_denoise_desc* desc, const sah_rtgi_denoise_params* params,
                     uint32_t row_begin, uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_RTGI_DENOISE_H */
