/* sah_sun_shafts.h — volumetric sun light: the in-scattering of the sun in a homogeneous medium between the camera and the geometry, marched
 * through the cascaded shadow map that sah_shadow_render fills and sah_lighting reads.  The reference has no counterpart: it keeps a value
 * "used for volumetrics, which I will totally code up at some point" (render/gi/irradiance_cache.hpp:172) and its sky shaders leave the
 * medium between camera and geometry out.  This pass is builder-owned, like sah_ssr, sah_sharpen, sah_exposure_* and sah_motion_blur: its
 * arithmetic is fixed below ("ABI-defined"), restated in numpy by tests/sun_shafts_ref.py and pinned bit for bit by
 * tests/golden/sun_shafts_*.npz.  Parity unpinned.  Off by default everywhere: nothing in the library, in include/sah_host.hpp or in
 * androidrenderer_amd/frame.py runs it unless the caller asks.  Its place is between Lighting and the anti-aliasing (Lighting -> sun shafts
 * -> SSR -> TAA ...), where the temporal resolve absorbs its dither.  Not part of sah_chain_*.  Same conventions as sah_hip.h (this header
 * includes it).
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing, leaves its inputs and every cache and epoch of
 * the context untouched, and may be recorded under stream capture.
 */
#ifndef SAH_SUN_SHAFTS_H
#define SAH_SUN_SHAFTS_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_SUN_SHAFTS_DITHER 1u    /* the samples of a march texel are shifted along its ray by the 4 x 4 ordered matrix (below) */
#define SAH_SUN_SHAFTS_TERM_ONLY 2u /* `out` gets (S, T), the term and the transmittance, and `lit` is not read (it may be NULL) */

/* 60 bytes, host memory, read during the call. */
typedef struct sah_sun_shafts_params {
    float step_length;        /* length of a march step in view-space units, finite and > 0; default 0.5 */
    uint32_t num_steps;       /* steps of a ray, 1..64; default 32 */
    float step_transmittance; /* tau, the share of light that survives one step, in (0, 1]; exp(-extinction * step_length), formed by the
                                 caller: the library never evaluates an exponential; default 0.98 */
    float albedo[3];          /* scattering albedo, finite; the sun's colour is in Lighting's units, so a caller whose `lit` came out of
                                 sah_lighting folds Lighting's exposure constant 0.00031415927 in here; default 1 */
    float ambient[3];         /* unshadowed in-scatter per unit of extinguished light, in lit's units, finite; default 0 */
    float anisotropy;         /* g of the Henyey-Greenstein phase function, in (-1, 1); default 0.6 */
    float depth_bias;         /* subtracted from the sample's shadow-map depth before the compare, finite; default 0.0005 */
    float depth_sharpness;    /* of the depth-aware upsample under downscale 2, finite and >= 0; default 50 */
    uint32_t downscale;       /* s: 1 or 2, the march runs on every s-th pixel of every s-th row; default 1 */
    uint32_t dither_offset;   /* 0..15, added to the matrix entry modulo 16 (a caller steps it per frame); default 0 */
    uint32_t flags;           /* SAH_SUN_SHAFTS_*; default 0 */
} sah_sun_shafts_params;
#define SAH_SUN_SHAFTS_DEFAULT_STEP_LENGTH 0.5f
#define SAH_SUN_SHAFTS_DEFAULT_NUM_STEPS 32u
#define SAH_SUN_SHAFTS_DEFAULT_STEP_TRANSMITTANCE 0.98f
#define SAH_SUN_SHAFTS_DEFAULT_ALBEDO 1.0f
#define SAH_SUN_SHAFTS_DEFAULT_AMBIENT 0.0f
#define SAH_SUN_SHAFTS_DEFAULT_ANISOTROPY 0.6f
#define SAH_SUN_SHAFTS_DEFAULT_DEPTH_BIAS 0.0005f
#define SAH_SUN_SHAFTS_DEFAULT_DEPTH_SHARPNESS 50.0f
#define SAH_SUN_SHAFTS_DEFAULT_DOWNSCALE 1u
#define SAH_SUN_SHAFTS_DEFAULT_DITHER_OFFSET 0u
#define SAH_SUN_SHAFTS_DEFAULT_FLAGS 0u
#define SAH_SUN_SHAFTS_MAX_STEPS 64u

/* lit, out: R16G16B16A16_SFLOAT, w x h (the render resolution).  depth: D32_SFLOAT, reversed Z, w x h.  shadowmap: what sah_lighting takes
 * in CSM mode, D16_UNORM or D32_SFLOAT, one layer per cascade; its first min(depth, 4) layers are the cascades the pass knows, and a NULL
 * shadowmap (or a NULL ptr) means every sample is lit.  march: R16G16B16A16_SFLOAT caller-owned scratch, mw x mh = ceil(w / s) x ceil(h / s),
 * written by the call: rgb the in-scattered light S, a the transmittance T.  w, h < 2^31 and w * h < 2^32; the shadow map's layer below 4 GiB.
 *
 * In fp32, every operator rounded on its own (no contraction anywhere), IEEE division and square root, no transcendental on the device.
 * All of it is ABI-defined.  clamp01(a) = a > 0 ? (a < 1 ? a : 1) : 0 (a NaN gives 0).  M * v is sah_lighting's product: row r is
 * ((M[r] v.x + M[4 + r] v.y) + M[8 + r] v.z) + M[12 + r] v.w.  half(v) rounds to nearest even, and a NaN is stored as 0x7E00.
 * Host       nf = float(num_steps).  P[0] = 1, P[k + 1] = P[k] * tau, D[k] = P[k] - P[k + 1] for k < num_steps: the share of a ray's energy
 *            that step k removes (tau = 1: D = 0).  d_min = z_near / (step_length * nf).  l = n * (1 / sqrt((n.x n.x + n.y n.y) + n.z n.z)) with
 *            n = -direction_and_tan_size.xyz (Lighting's direction towards the sun) and lv = mat3(view) * l, row r
 *            (view[r] l.x + view[4 + r] l.y) + view[8 + r] l.z.  A = inverse_view * (0, 0, 0, 1), the world position of the camera.
 *            biased_c = biasMat * cascade_matrices[c] exactly as sah_lighting forms it; a_c = (biased_c * (A, 1)).xyz / its w.
 *            g1 = 1 + g * g, g2 = 1 - g * g, g3 = 2 * g.
 * Texel      March texel (mx, my) stands for render pixel (x, y) = (s mx, s my), always inside the image.  d = depth[y][x];
 *            d_eff = d > d_min ? d : d_min: the sky (0), a NaN, a negative and a denormal depth all march the full num_steps * step_length.
 *            tx = (float(x) + 0.5) / float(w), ty likewise; ndc = (tx * 2 - 1, ty * 2 - 1, d_eff, 1); v = inverse_projection * ndc;
 *            e = v.xyz / v.w, the view-space end point (directional_light.rt.slang's reconstruction, with the plane's extent for the
 *            view's render_resolution); L = sqrt((e.x e.x + e.y e.y) + e.z e.z).  B = inverse_view * (e, 1).  For each cascade c < 4:
 *            b_c = (biased_c * B).xyz / its w and delta_c = b_c - a_c.  The cascades are orthographic, and the pass interpolates the
 *            DIVIDED end points: a sample costs a product and a sum per coordinate, no matrix and no divide.
 *            n = L / step_length and r = step_length / L, once per texel.  (Two divides per texel, where ((k + o frac) step_length) / L
 *            and (L - k step_length) / step_length would be two IEEE divides per sample for the same quantities.)
 * Dither     o = 0.5 without SAH_SUN_SHAFTS_DITHER; with it o = (float((b + dither_offset) & 15) + 0.5) * 0.0625, b = sah_ssr.h's matrix
 *            0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5 at [my & 3][mx & 3]: indexed by the MARCH texel, so that under s = 2 all sixteen
 *            offsets occur (the render pixel's coordinates are even there).
 * Sample     k = 0 .. num_steps - 1, each from its index: frac = clamp01(n - float(k)), the share of step k in front of the surface;
 *            t = (float(k) + o * frac) * r, the sample at the share o of the part of the step that is in front of the surface; zv = e.z * t; cascade = 0, then for i = 0..3 in order: zv < data[i][0] sets cascade = i + 1 (Lighting's
 *            selection).  sp = a_c + delta_c * t for c = cascade.  vis = 1 when cascade >= min(layers, 4), when a coordinate of sp is < 0,
 *            > 1 or a NaN, or without a shadow map; otherwise ref = sp.z - depth_bias, clamped to [0, 1] for D16_UNORM (ref < 0 ? 0 :
 *            ref > 1 ? 1 : ref), and vis = Lighting's bilinear compare at (sp.x, sp.y, layer c): the four texels around
 *            sp.xy * extent - 0.5, CLAMP_TO_EDGE per tap, D16 texels as float(v) / 65535, each compared ref < texel, and
 *            vis = (((1 - fx)(1 - fy) c00 + fx (1 - fy) c10) + (1 - fx) fy c01) + fx fy c11.
 * Sums       From E = V = 0, k ascending: E = E + frac * D[k]; V = V + (vis * frac) * D[k].  (A sample with frac == 0 adds +0.)
 * Phase      c = ((e.x / L) lv.x + (e.y / L) lv.y) + (e.z / L) lv.z; q = g1 - g3 * c; ph = (g2 / (q * sqrt(q))) * 0.07957747 (1 / 4 pi).
 * Term       T = 1 - E; S.c = E * ambient.c + (ph * sun.color.c) * (albedo.c * V).  march[my][mx] = half(S.rgb), half(T).
 * Composite  reads the STORED halfs of march, widened.  s = 1: (S', T') = march[y][x].  s = 2: X0 = x >> 1, X1 = min(X0 + 1, mw - 1),
 *            fx = x odd ? 0.5 : 0, likewise y; the four texels j = (X0, Y0), (X1, Y0), (X0, Y1), (X1, Y1) with the bilinear weights
 *            bw = (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy; z = z_near / d_eff of the pixel, z_j the same at texel j's render
 *            pixel, read from `depth`; W_j = bw_j * (1 / (1 + (depth_sharpness * |z - z_j|) / z)); sum = ((W_0 + W_1) + W_2) + W_3;
 *            T' = (((W_0 T_0 + W_1 T_1) + W_2 T_2) + W_3 T_3) / sum, S' likewise per channel.
 *            o.c = float(lit.c) * T' + S'.c; out = half(o.rgb) with lit's alpha bits.  The pixel stores lit's four halfs bit for bit when
 *            T' == 1 and S' == (0, 0, 0) — tau = 1 is the identity — and when a channel of o is not finite.
 *            Under SAH_SUN_SHAFTS_TERM_ONLY out = half(S'.rgb), half(T') (s = 1: the texel of march itself).
 *
 * Every plane 4-byte aligned with a pitch that is a multiple of 4 (the rules of sah_taa_resolve); the shadow map aligned to its texel, its
 * pitches multiples of its texel.
 *
 * Rows [row_begin, row_end) of `out` are written ((0, 0) = all rows), and a pixel's value does not depend on the row window.  A non-empty
 * band writes rows row_begin .. row_end - 1 of march under s = 1 and rows row_begin / 2 .. min((row_end - 1) / 2 + 1, mh - 1) under s = 2,
 * each in full.  An empty band writes and launches nothing.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane or a shadow map of another format; SAH_ERR_INVALID_ARGUMENT for a
 * NULL view, sun, params, depth, march, out or (without TERM_ONLY) lit, a NULL plane pointer, a zero extent, depth, lit and out not
 * sharing one extent, march other than ceil(w / s) x ceil(h / s), 2^32 texels or more, a pitch smaller than a row, a misaligned plane,
 * a shadow map with no layer, a zero extent, a short or misaligned pitch or a layer of 4 GiB or more, row_begin > row_end or row_end > h,
 * a step_length or z_near that is not finite and > 0, num_steps outside 1..64, step_transmittance outside (0, 1], an albedo, ambient,
 * depth_bias that is not finite, anisotropy outside (-1, 1), a depth_sharpness that is not finite and >= 0, downscale other than 1 or 2,
 * dither_offset above 15, a NaN in any parameter, an undefined flag bit, the byte range of `out` overlapping depth, lit or march, and
 * march overlapping depth or lit. */
int sah_sun_shafts(sah_ctx* ctx, const sah_view_data* view, const sah_sun_light_constants* sun, const sah_volume* shadowmap, const sah_plane* depth,
                   const sah_plane* lit, const sah_plane* march, const sah_plane* out, const sah_sun_shafts_params* params, uint32_t row_begin,
                   uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_SUN_SHAFTS_H */
