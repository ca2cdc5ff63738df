/* sah_sharpen.h — contrast-adaptive sharpening: the step between the upscaled (or antialiased) scene and auto-exposure, bloom and tonemap.
 *
 * The reference's default anti-aliasing is a vendor binary (r.AntiAliasing, scene_renderer.cpp) that does two things: a temporal upscale and
 * a contrast-adaptive sharpening pass over the upscaled image.  sah_taa_resolve and sah_taa_upscale stand in for the first; both low-pass the
 * image (a bilinear history tap, frame over frame).  This pass stands in for the second.  It is builder-owned, like sah_taa_resolve,
 * sah_ssao and sah_exposure: a plus-shaped five-tap filter with one negative lobe per pixel, limited so that the result stays inside the
 * range of the pixel's neighbourhood, evaluated on a range-compressed copy of the HDR scene.  Its arithmetic is fixed below ("ABI-defined"),
 * restated in numpy by tests/sharpen_ref.py and pinned bit for bit by tests/golden/sharpen_*.npz.  Parity unpinned: there is no reference
 * output to compare with.  Same conventions as sah_hip.h (this header includes it through sah_exposure.h).
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing, leaves every cache and epoch of the context
 * untouched, and may be recorded under stream capture (one kernel).
 *
 * NOT part of it: sah_chain_* integration; fusing with sah_taa_upscale or sah_exposure_meter; a 3 x 3 or wider neighbourhood; any change to
 * an existing pass.
 */
#ifndef SAH_SHARPEN_H
#define SAH_SHARPEN_H

#include "sah_exposure.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_SHARPEN_DENOISE 1u /* scale the lobe down where the centre looks like noise against its ring */

/* 12 bytes, host memory, read during the call. */
typedef struct sah_sharpen_params {
    float sharpness; /* in [0, 1]; 0 = no sharpening (see "Identity"), 1 = the full lobe; default 1 */
    float pre_scale; /* finite, > 0; default 1: the scene is multiplied by it before the range compression and divided by it after */
    uint32_t flags;  /* SAH_SHARPEN_* */
} sah_sharpen_params;

/* All of the following is ABI-defined.  fp32, every operator rounded on its own, no contraction.  min(a, b) = a < b ? a : b,
 * max(a, b) = a > b ? a : b (with a NaN for a, the result is b), as in sah_exposure.h.
 * Scale      k = pre_scale.  With `exposure` non-NULL, k' = pre_scale * exposure->exposure, and k = k' iff k' is finite, k' >= 2^-20 and
 *            k' <= 2^20; otherwise k = pre_scale.  The exposure is a device value the host cannot check, so the rule is the kernel's.  It
 *            lets the pass run on the unexposed scene ahead of sah_exposure_meter: the last frame's exposure places the sharpening in a
 *            perceptual range without a host read-back.  (pre_scale itself is the caller's: a k beyond [2^-20, 2^20] may overflow the
 *            compression, and eligible pixels may then come out as NaN.)
 * Taps       b = (x, y - 1), d = (x - 1, y), e = (x, y), f = (x + 1, y), h = (x, y + 1) of `scene`, coordinates clamped to the IMAGE.
 * Eligible   a texel is CLEAN iff its three colour channels are finite and none is < 0 (-0 is clean; alpha is not looked at).  A pixel is
 *            ELIGIBLE iff its five taps are clean.  A pixel that is not eligible stores the 16-bit patterns of e's rgb: a NaN, an
 *            infinity or a negative texel passes through five pixels unchanged and spreads no further.
 * Compress   every tap on its own, per channel c' = float(c) * k; M = max(max(c'.r, c'.g), c'.b); t = c' / (1 + M): the reversible
 *            tonemap.  Every channel lands in [0, 1].  From here on b, d, e, f, h are the compressed taps.
 * Limiter    per channel  mn4 = min(min(min(b, d), f), h), mx4 = max(max(max(b, d), f), h),
 *              hit_min = mx4 > 0 ? min(mn4, e) / (4 * mx4) : 0
 *              hit_max = (1 - max(mx4, e)) / (4 * mn4 - 4)            (0 / 0 where mn4 is 1: the NaN loses the min below)
 *              lobe_c  = max(-hit_min, hit_max)
 *            lobe = max(-0.1875, min(max(max(lobe_r, lobe_g), lobe_b), 0)) * sharpness.
 * Noise      with SAH_SHARPEN_DENOISE: L(p) = (p.r * 0.5 + p.g) + p.b * 0.5; nz = ((L(b) + L(d)) + (L(f) + L(h))) * 0.25 - L(e);
 *            range = max(max(max(max(L(b), L(d)), L(e)), L(f)), L(h)) - min(min(min(min(L(b), L(d)), L(e)), L(f)), L(h));
 *            q = range > 0 ? min(|nz| / range, 1) : 0; lobe = lobe * (1 - q * 0.5).
 * Resolve    per channel  s = (lobe * ((b + d) + (f + h)) + e) / (4 * lobe + 1), then s = min(max(s, 0), 1).
 * Expand     m = min(max(max(s.r, s.g), s.b), 1 - 2^-17); o = min((s / (1 - m)) / k, 65504).
 * Store      rgb = half(o), round to nearest even; alpha is the 16 bits of e's alpha, always.
 *
 * For every eligible pixel o is finite and >= 0 (k within [2^-20, 2^20]).
 * Identity   with sharpness 0, k = 1 and every colour value at most 4096, `out` equals `scene` bit for bit, but for a clean -0, which
 *            comes out as +0.  Beyond 8192 the identity is lost to the cancellation in 1 - m; nothing is promised above 4096.
 *
 * scene, out: R16G16B16A16_SFLOAT, one extent W x H with W, H < 2^31 and W * H < 2^32, 4-byte aligned with pitches that are multiples of 4
 * and at least a row (the rules of sah_taa_resolve); when every pointer and pitch is a multiple of 16 the kernel takes the 16-byte path,
 * otherwise every access is a dword.  `exposure`: 16 bytes of device memory, 4-byte aligned, or NULL; only its first word is read.
 * Rows [row_begin, row_end) of `out` are written and nothing else, (0, 0) = all rows; an empty band launches nothing.  The written rows
 * read rows row_begin - 1 .. row_end of `scene`, clamped to the image, not to the band: the pass is row-shardable with one row of halo.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format; SAH_ERR_INVALID_ARGUMENT for a NULL scene, out or
 * params, zero or differing extents, a pitch smaller than a row, a misaligned plane or exposure, row_begin > row_end or row_end > H,
 * sharpness outside [0, 1] (a NaN fails), pre_scale not finite or not > 0, unknown flag bits, and any overlap of out's byte range with
 * scene's or with the 16 bytes of `exposure` (the pass reads neighbours: not in place). */
int sah_sharpen(sah_ctx* ctx, const sah_plane* scene, const sah_exposure_state* exposure, const sah_plane* out, const sah_sharpen_params* params,
                uint32_t row_begin, uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_SHARPEN_H */
