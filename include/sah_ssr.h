/* sah_ssr.h — screen-space reflections: the specular indirect light a lit frame of this library otherwise lacks.  The reference has no
 * counterpart: its LPV overlay forms a specular estimate and multiplies it by vec3(0) (gi/lpv/overlay.frag:113-151), its other GI overlays
 * are diffuse only, and its frame has "Other postprocessing // TODO" where reflections would go (scene_renderer.cpp:417-419).  This pass is
 * builder-owned, like sah_ssao and sah_sharpen: it reads what the library already produces (the G-buffer, the view constants, an RGBA16F lit
 * scene, the context's sRGB / UNORM decode table) and its arithmetic is fixed below ("ABI-defined"), restated in numpy by tests/ssr_ref.py and
 * pinned bit for bit by tests/golden/ssr_*.npz.  Parity unpinned: there is no reference output to compare with.  Off by default everywhere:
 * nothing in the library, in include/sah_host.hpp or in androidrenderer_amd/frame.py runs it unless the caller asks.  It is NOT a Hi-Z trace
 * over sah_mip_chain_generate's pyramid, has no temporal reprojection of its own, no cone tracing over a blurred source and no importance
 * sampling: one mirror ray per pixel, marched linearly in screen space.  Same conventions as sah_hip.h (this header includes it).
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing, leaves its inputs and every cache and epoch of
 * the context untouched, and may be recorded under stream capture.
 */
#ifndef SAH_SSR_H
#define SAH_SSR_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_SSR_JITTER 1u          /* the first sample is offset by b / 16 of a stride, b the 4 x 4 ordered-dither entry of (x & 3, y & 3) */
#define SAH_SSR_REFLECTION_ONLY 2u /* `out` holds the reflection term alone in rgb and its scalar weight in alpha (a denoiser, a debug view) */

/* 36 bytes, host memory, read during the call. */
typedef struct sah_ssr_params {
    float max_distance;  /* view-space length of the ray, finite and > 0; default 50 */
    float thickness;     /* view-space thickness of a surface, >= 0 (+inf allowed); default 0.5 */
    float stride_pixels; /* pixels between samples along the ray's major axis, finite and >= 1; default 4 */
    uint32_t max_steps;  /* most samples per ray, 1..256; default 64 */
    uint32_t refine_steps; /* bisection steps after a hit, 0..8; default 4 */
    float max_roughness; /* roughness at which the reflection has faded out, in (0, 1]; default 0.6 */
    float edge_fade;     /* width of the faded band at the image's borders as a fraction of the screen, in (0, 0.5]; default 0.1 */
    float intensity;     /* scale of the reflection, finite and >= 0; default 1 */
    uint32_t flags;      /* SAH_SSR_*; default 0 */
} sah_ssr_params;
#define SAH_SSR_DEFAULT_MAX_DISTANCE 50.0f
#define SAH_SSR_DEFAULT_THICKNESS 0.5f
#define SAH_SSR_DEFAULT_STRIDE_PIXELS 4.0f
#define SAH_SSR_DEFAULT_MAX_STEPS 64u
#define SAH_SSR_DEFAULT_REFINE_STEPS 4u
#define SAH_SSR_DEFAULT_MAX_ROUGHNESS 0.6f
#define SAH_SSR_DEFAULT_EDGE_FADE 0.1f
#define SAH_SSR_DEFAULT_INTENSITY 1.0f

/* Per pixel (x, y) of a W x H frame, in fp32, every operator rounded on its own (no fma anywhere), IEEE division and square root.  All of
 * it is ABI-defined.  Written out: clamp01(a) = a > 0 ? (a < 1 ? a : 1) : 0 (a NaN gives 0), min(a, b) = a < b ? a : b, |a| clears the sign.
 * View       as sah_ssao.h: the projection SceneView produces; the pass reads P00 = projection[0], P11 = projection[5], P20 = projection[8],
 *            P21 = projection[9], z_near and the 3 x 3 of `view`.  The host forms ipx = 1 / P00, ipy = 1 / P11, tx = 2 / float(W),
 *            ty = 2 / float(H), hw = 0.5 * float(W), hh = 0.5 * float(H) once.
 * Surface    Depth, Position and Centre of sah_ssao.h: a texel with !(depth > 0) has no surface, otherwise z = z_near / depth,
 *            P = ((z * (ndc.x + P20)) * ipx, (z * (ndc.y + P21)) * ipy, -z) and N = v / l, the unit view-space normal.  With luts the 512-entry
 *            table of the context (256 sRGB -> linear, then i / 255): rough = luts[256 + data.g], metal = luts[256 + data.b],
 *            base.c = luts[color.c], f0.c = 0.04 + (base.c - 0.04) * metal for c of r, g, b.  The pixel PASSES THROUGH — `out` gets the four
 *            halfs of `lit` bit for bit, or four zeros under SAH_SSR_REFLECTION_ONLY — when it has no surface, when a component of P or N
 *            is not finite, when !(rough < max_roughness), or when intensity == 0.
 * Ray        pl = sqrt((P.x * P.x + P.y * P.y) + P.z * P.z); V = P / pl (three divisions); nv = (N.x * V.x + N.y * V.y) + N.z * V.z;
 *            nv2 = 2 * nv; R.c = V.c - nv2 * N.c.  len = max_distance, and when R.z > 0 (the ray returns towards the camera):
 *            lim = (z - z_near) / R.z, len = lim < len ? lim : len — clipped at the near plane, not dropped.  E.c = P.c + R.c * len;
 *            ze = -E.z, ze = ze > z_near ? ze : z_near.  A view-space point Q of linear depth zq lies at the pixel coordinates
 *            s.x = (((Q.x * P00) / zq - P20) + 1) * hw, s.y = (((Q.y * P11) / zq - P21) + 1) * hh: s0 from (P, z), s1 from (E, ze).
 *            k0 = 1 / z, k1 = 1 / ze; ds = s1 - s0, dk = k1 - k0; L = max(|ds.x|, |ds.y|) = |ds.x| > |ds.y| ? |ds.x| : |ds.y|.  The ray is a
 *            MISS unless |ds.x| < inf, |ds.y| < inf, L >= 1 and k0 < inf (a NaN fails).
 * Samples    jit = float(b) * 0.0625 with b = the matrix 0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5 at [y & 3][x & 3] under
 *            SAH_SSR_JITTER, otherwise 0.  For i = 1 .. max_steps, each from its index and never by accumulation:
 *            t_i = ((float(i) + jit) * stride_pixels) / L; t_i > 1 ends the ray, a miss.  s_i = s0 + t_i * ds (per component),
 *            k_i = k0 + t_i * dk, zr_i = 1 / k_i.  Unless 0 <= s_i.x < float(W) and 0 <= s_i.y < float(H) the ray ends, a miss (a NaN
 *            fails).  The texel is (floor(s_i.x), floor(s_i.y)); without a surface the march continues; otherwise zt = z_near / depth
 *            of the texel, dz = zr_i - zt, and the sample is a HIT when dz >= 0 and dz <= thickness; any other sample (the ray in front
 *            of the surface, or behind it by more than the thickness) continues.  A ray that used all max_steps samples is a miss.
 * Refinement after the first hit, at index i: lo = t_(i-1) (the formula above at i - 1, also for i = 1), hi = t_i; refine_steps times:
 *            mid = (lo + hi) * 0.5; the sample at mid (s, k and zr formed from mid as above) passes when it is inside the image, its texel
 *            has a surface and zr >= zt; hi = mid when it passes, lo = mid otherwise.  t_hit = hi, and the hit texel (hx, hy) is the
 *            texel of the sample at hi.  The hit is REJECTED, a miss, unless each of the rgb halfs of source[hy][hx] is >= 0 and < inf
 *            (-0 is clean; sah_sharpen's rule: such texels spread no further) and the hit texel's unit view normal Nh (Centre) has
 *            (Nh.x * R.x + Nh.y * R.y) + Nh.z * R.z < 0 (a back face, or a NaN, is rejected).
 * Result     A miss passes through.  Otherwise m = 1 - clamp01(-nv); m2 = m * m; m5 = (m2 * m2) * m; F.c = f0.c + (1 - f0.c) * m5 (no pow
 *            enters the contract); rf = clamp01(1 - rough / max_roughness); u = (float(hx) + 0.5) / float(W), v likewise with H;
 *            e = min(min(u, 1 - u), min(v, 1 - v)); ef = clamp01(e / edge_fade); tf = clamp01(1 - t_hit); w = ((intensity * rf) * ef) * tf;
 *            g.c = w * F.c; out.c = half(float(lit.c) + g.c * float(source[hy][hx].c)), out.a = lit.a (its bits).  Under
 *            SAH_SSR_REFLECTION_ONLY out.c = half(g.c * float(source[hy][hx].c)) and out.a = half(w).  half() rounds to nearest even.
 *
 * color: R8G8B8A8_SRGB, normals: R16G16B16A16_SFLOAT (world space, unnormalised), data: R8G8B8A8_UNORM (g roughness, b metalness),
 * depth: D32_SFLOAT reversed Z — the four planes of sah_gbuffer the pass reads, handed over one by one as sah_ssao takes its two;
 * source, lit, out: R16G16B16A16_SFLOAT.  All W x H with W, H < 2^31 and W * H < 2^32.  `source` is the image the reflections are taken
 * from (this frame's lit scene, or last frame's output), `lit` the image they are added to; the two may be one plane.  `scratch`:
 * R32_SFLOAT, ceil(W / 8) x ceil(H / 8), always required and RESERVED: it is checked like every plane, and this version neither reads nor
 * writes it (it is where a per-block nearest depth would live; a caller that provides it needs no change when the pass starts using it).  Every plane 4-byte aligned with a
 * pitch that is a multiple of 4; when normals, lit and out are 8-byte aligned with pitches that are multiples of 8 the pass moves whole
 * texels, otherwise dwords — the bytes written are the same.  The library allocates nothing.
 *
 * Rows [row_begin, row_end) of `out` are written ((0, 0) = all rows), and a pixel's value does not depend on the row window.  A non-empty
 * band reads the same rows of color, normals, data and lit, ANY row of depth, normals and source (a ray goes where it goes).  A later
 * version may write the WHOLE of scratch in any non-empty band.  An empty band writes and launches nothing.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer,
 * zero or differing extents (scratch: other than ceil(W / 8) x ceil(H / 8)), a pitch smaller than a row, a misaligned plane,
 * row_begin > row_end or row_end > H, a max_distance that is not finite and positive, thickness < 0, a stride_pixels that is not finite
 * and >= 1, max_steps outside 1..256, refine_steps > 8, max_roughness outside (0, 1], edge_fade outside (0, 0.5], an intensity that is
 * not finite and >= 0, an undefined flag bit, a NaN in any parameter or in any field of `view` the pass reads, a z_near that is not
 * finite and positive, the byte range of `out` overlapping that of an input or of scratch, and scratch overlapping an input. */
int sah_ssr(sah_ctx* ctx, const sah_view_data* view, const sah_plane* color, const sah_plane* normals, const sah_plane* data,
            const sah_plane* depth, const sah_plane* source, const sah_plane* lit, const sah_plane* scratch, const sah_plane* out,
            const sah_ssr_params* params, uint32_t row_begin, uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_SSR_H */
