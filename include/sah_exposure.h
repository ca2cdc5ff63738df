/* sah_exposure.h — histogram auto-exposure: the step between the antialiased (or upscaled) scene and the bloom / tonemap pair.
 *
 * The reference fixes the lit scene's scale by literals (0.00031415927 in the sun pass, 3.1415927 for emission, 0.314159 / 0.0031415927 in
 * the GI paths, r.GI.LPV.Exposure) and marks the gap twice with the same TODO ("auto-exposure - Better exposure",
 * directional_light.frag:143, gi/lpv/overlay.frag:157): there is no shader to follow.  This pass is builder-owned, like sah_taa_resolve,
 * sah_ssao and sah_rt_denoise: it meters the frame's luminance with a 256-bin histogram, derives one exposure factor, and multiplies the
 * scene by it.  Its arithmetic is fixed below ("ABI-defined"), restated in numpy by tests/exposure_ref.py and pinned bit for bit by
 * tests/golden/exposure_*.npz.  Parity unpinned: there is no reference output to compare with.  The histogram is integer arithmetic, so the
 * result does not depend on the order in which pixels arrive.  Same conventions as sah_hip.h (this header includes it).
 *
 * Both calls run on the context's stream, do no host synchronisation, allocate nothing, leave every cache and epoch of the context
 * untouched, and may be recorded under stream capture (sah_exposure_meter: a linear chain of two kernels, the first of which zeroes `work`).
 *
 * NOT part of it: metering a row window, or combining histograms across the ranks of a sharded frame (the histogram is left in `work` so
 * that a later change can add this); sah_chain_* integration; spatial weighting or a sky mask; local exposure; any change to sah_tonemap,
 * sah_bloom or sah_lighting.
 */
#ifndef SAH_EXPOSURE_H
#define SAH_EXPOSURE_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_EXPOSURE_HISTORY_INVALID 1u /* first frame / after a cut: state_in is neither read nor checked and may be NULL */
#define SAH_EXPOSURE_BINS 256
#define SAH_EXPOSURE_WORK_BYTES 1040 /* 256 bins, one ticket word, three reserved words */

/* 32 bytes, host memory, read during the call.  The defaults are design choices, not measurements. */
typedef struct sah_exposure_params {
    float key;               /* luminance the metered average is mapped to; finite, > 0; default 0.18 */
    float low_fraction;      /* metering window of the cumulative histogram, 0 <= low < high <= 1; defaults 0.5, 0.95 */
    float high_fraction;
    float min_exposure;      /* finite, 0 < min <= max; defaults 1/64, 64 */
    float max_exposure;
    float adaptation;        /* weight of this frame's metered value, in (0, 1]; default 1 (the caller derives it from its frame time) */
    uint32_t max_workgroups; /* 0 = the library's choice; otherwise the grid is at most this many workgroups.  The result never depends on it */
    uint32_t flags;          /* SAH_EXPOSURE_* */
} sah_exposure_params;

/* 16 bytes of DEVICE memory, 4-byte aligned. */
typedef struct sah_exposure_state {
    float exposure;   /* the factor sah_exposure_apply multiplies by */
    float adapted;    /* adapted pseudo-log2 luminance (below); a NaN means "no history" */
    uint32_t metered; /* N: pixels in bins 1..255 */
    uint32_t window;  /* hi - lo */
} sah_exposure_state;

/* All of the following is ABI-defined.  fp32, every operator rounded on its own, no contraction.  bits(x) is the 32-bit pattern of the
 * float x.  f2u is the float-to-uint32 conversion: truncation; a NaN and negatives give 0, values of 2^32 and more give 2^32 - 1.
 * min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b (with a NaN for a, the result is b).
 * Luminance  c = rgb of scene[y][x], half -> float.  L = (c.r * 0.2126 + c.g * 0.7152) + c.b * 0.0722.  The pixel is COUNTED iff L is
 *            finite and L > 0.
 * Bin        eight bins per octave from 2^-20 to 2^12, taken from the bits of L, with no transcendental:
 *            k = clamp(int(bits(L) >> 20) - 856, 0, 255), 856 = (127 - 20) * 8; a subnormal L lands in bin 0.  n[k] += 1 for every counted
 *            pixel.  Bin 0 is the "black" bin: counted in the histogram, left out of the average.  The pseudo-log2 of a luminance is
 *            plog(L) = bits(L) / 2^23 - 127 (exact at powers of two, linear in the mantissa between); bin k covers
 *            [k / 8 - 20, (k + 1) / 8 - 20).
 * Window     N = sum of n[1..255] (W * H < 2^32: a uint32).  lo = min(f2u(float(N) * low_fraction), N), hi likewise from high_fraction;
 *            float(N) rounds to nearest even.  For b = 1..255 in order, with C the running sum of n[1..b-1] and
 *            cl(x) = min(max(x, lo), hi) on integers: c_b = cl(C + n[b]) - cl(C), S += uint64(c_b) * (2 b + 1).  S is exact in uint64.
 * Metered    the frame is METERED iff hi > lo.  Then m_t = (float(S) / float(hi - lo)) * 0.0625 - 20.0, uint64 -> float and
 *            uint32 -> float rounded to nearest even, IEEE division: the mean over the window of the bins' centres, as a pseudo-log2.
 * Adaptation the history is valid iff SAH_EXPOSURE_HISTORY_INVALID is clear and state_in->adapted is finite; that value is m_p.
 *              metered, history valid      m = m_p + (m_t - m_p) * adaptation
 *              metered, history invalid    m = m_t
 *              not metered, history valid  m = m_p
 *              not metered, invalid        none: exposure = min(max(1.0, min_exposure), max_exposure), adapted = the quiet NaN 0x7fc00000
 * Exposure   L_avg = bitcast<float>(f2u((m + 127.0) * 8388608.0)), e = key / L_avg (IEEE division),
 *            exposure = min(max(e, min_exposure), max_exposure).  state_out = {exposure, m, N, hi - lo}.  state_out may be the same address
 *            as state_in: one thread reads it, then writes it.
 * Apply      out.rgb = half(float(scene.rgb) * state->exposure), round to nearest even, overflow to infinity; alpha keeps its 16 bits.
 *
 * sah_exposure_meter meters the whole of `scene`.  With `exposed_out` non-NULL it also writes, in the same pass over `scene`, exactly what
 * sah_exposure_apply(scene, state_in, exposed_out, 0, 0) writes (the fused form): the usual one-frame latency — the frame is exposed by
 * what the last frame metered, and the metering reads the unexposed scene.  The fused form is refused together with
 * SAH_EXPOSURE_HISTORY_INVALID: the first frame calls meter, then apply.
 *
 * `work`: caller-owned device memory of SAH_EXPOSURE_WORK_BYTES, 4-byte aligned.  Its contents on entry do not matter: the call zeroes it
 * on the stream first.  After the call words 0..255 hold the frame's histogram n[0..255]; the rest is unspecified.
 *
 * scene, out, exposed_out: R16G16B16A16_SFLOAT, one extent W x H with W, H < 2^31 and W * H < 2^32, 4-byte aligned with pitches that are
 * multiples of 4 and at least a row; when every plane's pointer and pitch is a multiple of 16 the kernel takes the 16-byte path.  `out`
 * (`exposed_out`) may be exactly the plane `scene` (same pointer and pitch), or its byte range is disjoint from it.
 * sah_exposure_apply writes rows [row_begin, row_end) of `out` ((0, 0) = all rows) and nothing else; an empty band launches nothing.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer
 * (`state_in` may be NULL only with SAH_EXPOSURE_HISTORY_INVALID, `exposed_out` always), zero or differing extents, a pitch smaller than a
 * row, a misaligned plane, state or `work`, row_begin > row_end or row_end > H, key, min_exposure or max_exposure not finite and > 0,
 * min_exposure > max_exposure, fractions that are not 0 <= low < high <= 1 (a NaN fails), adaptation outside (0, 1], unknown flag bits,
 * `exposed_out` with SAH_EXPOSURE_HISTORY_INVALID, and any overlap among `work`, `state_out`, `state_in` (other than
 * state_in == state_out) and the planes, beyond what is allowed above. */
int sah_exposure_meter(sah_ctx* ctx, const sah_plane* scene, const sah_exposure_state* state_in, sah_exposure_state* state_out, void* work,
                       const sah_plane* exposed_out, const sah_exposure_params* params);
int sah_exposure_apply(sah_ctx* ctx, const sah_plane* scene, const sah_exposure_state* state, const sah_plane* out, uint32_t row_begin,
                       uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_EXPOSURE_H */
