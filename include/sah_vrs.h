/* sah_vrs.h — the two consumers of the shading-rate image that sah_vrsaa.h produces: Lighting at the rate the image asks for, and the
 * resolve of the 2W x 2H frame of AntiAliasingType::VRSAA down to the output.
 *
 * The reference renders the mode at twice the output resolution and stops there: `// TODO: Perform a proper VSR resolve, and also do VRS in
 * lighting` (RenderCore/render/scene_renderer.cpp:142-154, 476-481); it never writes `antialiased_scene`.  It fixes nothing of either pass,
 * so every rule below is ABI-defined.  The rules are chosen so that no new shading arithmetic exists: every pixel sah_lighting_vrs writes
 * is, bit for bit, the value sah_lighting writes at some pixel of the same frame.  Same conventions as sah_hip.h (this header includes it
 * through sah_vrsaa.h).
 *
 * Both calls run on the context's stream, do no host synchronisation, allocate nothing, leave their inputs and every cache, epoch and the
 * sah_debug_lighting_dispatch record of the context untouched, and may be recorded under stream capture.
 */
#ifndef SAH_VRS_H
#define SAH_VRS_H

#include "sah_vrsaa.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sah_lighting_vrs_desc {
    const sah_lighting_desc* lighting;   /* exactly what sah_lighting takes */
    const sah_plane* shading_rate_image; /* R8_UINT (SAH_FORMAT_R8_UINT), what sah_vrsaa_shading_rate_image writes */
    uint32_t texel_size[2];              /* pixels of `lit` per texel of the image, per axis */
    float depth_tolerance;
} sah_lighting_vrs_desc;

/* Lighting at a variable rate.  Per pixel q = (x, y) of the W x H plane `lit` of desc->lighting (all ABI-defined):
 *
 * Rate        c is the byte at texel (x / texel_size[0], y / texel_size[1]) of the shading-rate image.  lw = min((c >> 2) & 3, 2) and
 *             lh = min(c & 3, 2): Vulkan's code, the one sah_vrsaa_shading_rate_image stores.  ABI-defined: a field value of 3 counts as
 *             2, and bits 4-7 are ignored.
 * Coarse      ABI-defined: the box with origin (x & ~(2^lw - 1), y & ~(2^lh - 1)) and extent 2^lw x 2^lh, cut at the image's right and
 * pixel       bottom edges.  Texel sizes are multiples of 4, so it lies within one texel of the image.
 * Surface     ABI-defined: `depth != 0.0f` as IEEE has it (NaN is a surface, -0 is not) — the test every lighting stage uses.
 * Represen-   ABI-defined: r is the first surface pixel of the coarse pixel in row-major order, or none.
 * tative
 * Source      ABI-defined: s(q) = r where q is a surface pixel, r exists, and fabsf(d_q - d_r) <= depth_tolerance * fabsf(d_r), evaluated
 *             in fp32 with every operator rounded on its own; a NaN compares false.  Otherwise s(q) = q: pixels that are not surface
 *             always shade themselves (the emissive add and the sky fill), and so do surface pixels whose depth is too far from the
 *             representative's — the rate image is a frame old, and this keeps a stale coarse rate from smearing across a new edge.
 *             s(r) = r.  depth_tolerance = +infinity shares whenever the compare is defined (a NaN depth on either side, two equal
 *             infinities, and a tolerance of 0 under an infinite representative leave it undefined).
 * Result      ABI-defined: the eight bytes at q are the eight bytes sah_lighting(ctx, desc->lighting) writes at s(q).  That is the whole
 *             contract.  Coarse shading of sky pixels is deliberately left out: the sun disc has no contrast in the G-buffer, so it
 *             would get the coarsest rate.
 *
 * Supported (ABI-defined): sun off, CSM or RT, with GI none or LPV; sky, AO plane, shadow mask and flags as in sah_lighting.
 * SAH_ERR_UNSUPPORTED, before any launch, for GI kinds CACHE and RTGI and for a non-empty light list.
 *
 * Rows (ABI-defined): the range is row_begin / row_end of desc->lighting, (0, 0) = all rows.  row_begin must be a multiple of 4; row_end
 * a multiple of 4 or H.  A coarse pixel then never straddles a shard's edge, so the sharded frame is the unsharded frame.  Rows outside
 * the range are not written.
 *
 * Before anything is launched: everything sah_lighting refuses, with its codes; SAH_ERR_UNSUPPORTED_FORMAT for a shading-rate image that
 * is not R8_UINT; SAH_ERR_INVALID_ARGUMENT for a NULL pointer, a texel size that is not a power of two in [4, 64], a shading-rate image
 * smaller than ceil(W / texel_size[0]) x ceil(H / texel_size[1]) (a larger one is accepted), a pitch below its width, a depth_tolerance
 * that is negative or NaN, and a row range that breaks the rule above. */
int sah_lighting_vrs(sah_ctx* ctx, const sah_lighting_vrs_desc* desc);

/* The resolve of the VRSAA frame: `lit` is 2W x 2H R16G16B16A16_SFLOAT, `antialiased` is W x H of the same format (all ABI-defined).
 *
 * Per channel ((a + b) + (c + d)) * 0.25f in fp32, every operator rounded, no fma; a, b are the upper pair of the pixel's 2 x 2 block of
 *             `lit`, left first; c, d the lower pair.
 * Store       as a half, round to nearest even (overflow to infinity cannot happen: the mean of four halfs is in range).  A NaN is
 *             stored as the positive quiet NaN 0x7e00.
 * Rows        [row_begin, row_end) of `antialiased`, (0, 0) = all rows.  Any extent the planes can describe is accepted.
 *
 * Both planes 8-byte aligned with pitches that are multiples of 8.  Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of
 * another format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer, a zero extent, a source that is not exactly twice the target per axis (odd
 * source extents included), a pitch smaller than a row, a misaligned plane, planes that overlap, row_begin > row_end or row_end > H. */
int sah_vrsaa_resolve(sah_ctx* ctx, const sah_plane* lit, const sah_plane* antialiased, uint32_t row_begin, uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_VRS_H */
