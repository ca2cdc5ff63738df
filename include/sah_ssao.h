/* sah_ssao.h — screen-space ambient occlusion: the third way the reference fills its AO target (r.AO: Off, CACAO, RTAO,
 * RenderCore/render/phase/ambient_occlusion_phase.cpp:157-189).  sah_ao_clear is Off and sah_rtao is RTAO (sah_hip.h); CACAO is a vendor SDK:
 * there is no shader to follow.  This pass is builder-owned, like sah_taa_resolve: it reads what the CACAO call reads (depth, G-buffer
 * normals, the view's projection and view matrices), writes what it writes (the R32_SFLOAT AO plane that sah_lighting's LPV overlay
 * consumes), and its settings carry the names and defaults the reference gives CACAO (ambient_occlusion_phase.cpp:302-320).  Its arithmetic
 * is fixed below ("ABI-defined"), restated in numpy by tests/ssao_ref.py and pinned bit for bit by tests/golden/ssao_*.npz.  Parity
 * unpinned: there is no reference output to compare with.  It is NOT a CACAO port: no adaptive quality, no deinterleaved or half-resolution
 * sampling, no normals generated from depth, no bent normals, no temporal accumulation.  Same conventions as sah_hip.h (this header
 * includes it).
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing, leaves its inputs and every cache and epoch of
 * the context untouched, and may be recorded under stream capture.
 */
#ifndef SAH_SSAO_H
#define SAH_SSAO_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 40 bytes, host memory, read during the call.  The defaults are the reference's CACAO settings. */
typedef struct sah_ssao_params {
    float radius;                     /* world units, finite and > 0; r.AO.MaxRayDistance, 8 */
    float max_radius_pixels;          /* cap of the sampling radius on screen, >= 1; default 32 */
    float shadow_multiplier;          /* 1 */
    float shadow_clamp;               /* in [0, 1]; 0.98 */
    float horizon_angle_threshold;    /* in [0, 1]; 0.06 */
    float fade_out_from, fade_out_to; /* view-space distances, from < to; 50, 300 */
    float edge_sharpness;             /* blur: a neighbour whose relative depth difference reaches 1 / edge_sharpness has no weight; default 50 */
    uint32_t blur_passes;             /* 0, 1 or 2; the reference sets 2 */
    uint32_t flags;                   /* none defined yet: must be 0 */
} sah_ssao_params;

/* The two tables, exact fp32 values (computed in fp64, rounded once, written as hex floats).
 * SAH_SSAO_OFFSETS: tap k of 16 in the unit disc, a spiral: radius sqrt((k + 0.5) / 16), angle k * pi * (3 - sqrt(5)) (the golden angle).
 * SAH_SSAO_ROTATIONS: (cos, sin) of rotation j = (x & 3) + 4 * (y & 3), CACAO's 4 x 4 rotation idea: the angle is 2 pi b / 16 with b the
 * 4 x 4 ordered-dither matrix 0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5; the quarter turns are exact. */
#define SAH_SSAO_TAPS 16
#define SAH_SSAO_OFFSETS                                   \
    {                                                      \
        {0x1.6a09e6p-3f, 0x0p+0f},                         \
        {-0x1.ce61a6p-3f, 0x1.a7944cp-3f},                 \
        {0x1.1b197cp-5f, -0x1.9338cp-2f},                  \
        {0x1.2366a4p-2f, 0x1.7c14b6p-2f},                  \
        {-0x1.0b60d6p-1f, -0x1.7a5d16p-4f},                \
        {0x1.fa916ep-2f, -0x1.423cb6p-2f},                 \
        {-0x1.52dfccp-3f, 0x1.3b2618p-1f},                 \
        {-0x1.43228cp-2f, -0x1.37169ep-1f},                \
        {0x1.5e896ap-1f, 0x1.0007ecp-2f},                  \
        {-0x1.6cacd4p-1f, 0x1.2d10bp-2f},                  \
        {0x1.5f9852p-2f, -0x1.77ab48p-1f},                 \
        {0x1.03d1dcp-2f, 0x1.9e2c56p-1f},                  \
        {-0x1.878cc6p-1f, -0x1.c5d284p-2f},                \
        {0x1.cb5526p-1f, -0x1.93ee94p-3f},                 \
        {-0x1.1852d4p-1f, 0x1.8ebb3cp-1f},                 \
        {-0x1.030b8p-3f, -0x1.f3c208p-1f},                 \
    }
#define SAH_SSAO_ROTATIONS                                 \
    {                                                      \
        {0x1p+0f, 0x0p+0f},                                \
        {-0x1p+0f, 0x0p+0f},                               \
        {0x1.6a09e6p-1f, 0x1.6a09e6p-1f},                  \
        {-0x1.6a09e6p-1f, -0x1.6a09e6p-1f},                \
        {0x0p+0f, -0x1p+0f},                               \
        {0x0p+0f, 0x1p+0f},                                \
        {0x1.6a09e6p-1f, -0x1.6a09e6p-1f},                 \
        {-0x1.6a09e6p-1f, 0x1.6a09e6p-1f},                 \
        {0x1.87de2ap-2f, 0x1.d906bcp-1f},                  \
        {-0x1.87de2ap-2f, -0x1.d906bcp-1f},                \
        {0x1.d906bcp-1f, 0x1.87de2ap-2f},                  \
        {-0x1.d906bcp-1f, -0x1.87de2ap-2f},                \
        {0x1.d906bcp-1f, -0x1.87de2ap-2f},                 \
        {-0x1.d906bcp-1f, 0x1.87de2ap-2f},                 \
        {0x1.87de2ap-2f, -0x1.d906bcp-1f},                 \
        {-0x1.87de2ap-2f, 0x1.d906bcp-1f},                 \
    }

/* Per pixel (x, y) of a W x H frame, in fp32, every operator rounded on its own (no fma anywhere), IEEE division and square root.  All of
 * it is ABI-defined.  Written out: clamp01(a) = a > 0 ? (a < 1 ? a : 1) : 0 and max0(a) = a > 0 ? a : 0 (a NaN gives 0),
 * min(a, b) = a < b ? a : b.
 * View       The pass assumes the projection SceneView produces — infinite reversed Z with the jitter in column 2
 *            (RenderCore/render/scene_view.cpp:13-27,163-164) — and reads only P00 = projection[0], P11 = projection[5], P20 = projection[8],
 *            P21 = projection[9], z_near, and the 3 x 3 of `view` (column major: m[0..2], m[4..6], m[8..10]).  The host forms ipx = 1 / P00,
 *            ipy = 1 / P11, tx = 2 / float(W), ty = 2 / float(H), sx = (0.5 * float(W)) * P00 and rs = radius * sx once.
 * Depth      a texel with !(depth > 0) (sky, NaN, negative) has no surface.  Otherwise z = z_near / depth: one division per texel, against
 *            three for the inverse_projection route.
 * Position   of texel (x, y) with a surface: ndc.x = (float(x) + 0.5) * tx - 1, ndc.y = (float(y) + 0.5) * ty - 1,
 *            P = ((z * (ndc.x + P20)) * ipx, (z * (ndc.y + P21)) * ipy, -z).
 * Centre     n = the rgb halfs of normals[y][x] as floats; v_i = (m[i] * n.x + m[4 + i] * n.y) + m[8 + i] * n.z;
 *            l = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z); N = v / l (three divisions).  A pixel with no surface, or with a non-finite
 *            component of P or N, stores 1.0.
 * Radius     t = rs / z; r_px = t > 1 ? (t < max_radius_pixels ? t : max_radius_pixels) : 1; R = (r_px * z) / sx, the world reach actually
 *            sampled; RR = R * R.  The falloff uses R, so a capped radius does not leave occluders at full weight beyond the samples.
 * Taps       16, in ascending k.  e = (s.x * c - s.y * sn, s.x * sn + s.y * c) with s = SAH_SSAO_OFFSETS[k] and
 *            (c, sn) = SAH_SSAO_ROTATIONS[(x & 3) + 4 * (y & 3)] (e depends on k, x & 3, y & 3 only and may be tabulated).
 *            f.x = (float(x) + 0.5) + e.x * r_px, f.y likewise.  The tap is SKIPPED unless 0 <= f.x < float(W) and 0 <= f.y < float(H)
 *            (outside the image: skipped, not clamped; a NaN fails); its texel is (floor(f.x), floor(f.y)); it is skipped when that is the
 *            centre texel or has no surface.  S = the tap texel's Position; d = S - P; vv = (d.x * d.x + d.y * d.y) + d.z * d.z; skipped
 *            unless vv > 0 and vv < inf.  Otherwise ndotd = ((N.x * d.x + N.y * d.y) + N.z * d.z) / sqrt(vv),
 *            falloff = clamp01(1 - vv / RR), o = max0(ndotd - horizon_angle_threshold) * falloff, sum = sum + o (from +0), n = n + 1.
 *            (A pixel within r_px texels of the image's border averages the taps that remain, all to one side of it: next to an
 *            occluder its value differs from what the whole disc would give — DESIGN.md section 5q has a measured case.)
 * Result     n == 0 stores 1.0.  Otherwise fade = clamp01((fade_out_to - z) / (fade_out_to - fade_out_from)) (the divisor formed on the
 *            host), obs = min(((sum / float(n)) * shadow_multiplier) * fade, shadow_clamp), occ = 1 - obs, ao = occ * sqrt(occ): the
 *            reference's shadowPower of 1.5 is hard-wired as x * sqrt(x) so that no pow enters the contract.
 * Blur       blur_passes times, each pass reading the previous pass's plane a (the first: the raw result above).  A pixel with no surface
 *            stores 1.0.  Otherwise num = a_c, den = 1, and for the left, right, upper and lower neighbour in that order, where it lies
 *            inside the image and has a surface: w = max0(1 - (|z_n - z_c| / z_c) * edge_sharpness), num = num + w * a_n, den = den + w;
 *            the pixel stores num / den.
 *
 * depth: D32_SFLOAT, reversed Z as the G-buffer writes it; normals: R16G16B16A16_SFLOAT, world space, unnormalised (the G-buffer's);
 * scratch and ao_out: R32_SFLOAT.  All W x H with W, H < 2^31 and W * H < 2^32, 4-byte aligned with pitches that are multiples of 4 (the
 * rules of sah_taa_resolve); when depth, normals and the raw pass's target are 16-byte aligned with pitches that are multiples of 16 the
 * raw pass takes the 16-byte path.  `scratch` holds the raw (unblurred) result; it is needed only with blur_passes > 0 and is neither
 * read nor checked, and may be NULL, with blur_passes == 0.  The library allocates nothing.
 *
 * Rows [row_begin, row_end) of `ao_out` are written ((0, 0) = all rows), and a pixel's value does not depend on the row window.  With
 * b = blur_passes, a non-empty band writes rows [max(row_begin - b, 0), min(row_end + b, H)) of `scratch` (b > 0) and reads the same rows
 * of `normals`, and ANY row of `depth` (a tap reaches max_radius_pixels rows away).  An empty band writes and launches nothing.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer
 * (`scratch` may be NULL only with blur_passes == 0), zero or differing extents, a pitch smaller than a row, a misaligned plane,
 * row_begin > row_end or row_end > H, a non-finite or non-positive radius, max_radius_pixels < 1, shadow_clamp or horizon_angle_threshold
 * outside [0, 1], fade_out_from >= fade_out_to, blur_passes > 2, non-zero flags, a NaN in any parameter or in any field of `view` the
 * pass reads, a z_near that is not finite and positive, the byte range of `ao_out` or of `scratch` overlapping that of an input, and
 * `ao_out` overlapping `scratch`. */
int sah_ssao(sah_ctx* ctx, const sah_view_data* view, const sah_plane* depth, const sah_plane* normals, const sah_plane* scratch,
             const sah_plane* ao_out, const sah_ssao_params* params, uint32_t row_begin, uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_SSAO_H */
