/* sah_mip_chain.h — the mip-chain generator: AMD's single-pass downsampler (SPD) as the reference drives it, one launch that writes every
 * level of an image from a source image.  The reference builds its Hi-Z pyramid with it every frame.
 *
 * Host side: MipChainGenerator::fill_mip_chain, RenderCore/render/mip_chain_generator.cpp:60-177; called by DepthCullingPhase::render on
 * the depth buffer (render/phase/depth_culling_phase.cpp:164).  Shaders: RenderCore/shaders/util/mip_chain_generator_{D32F_min, R16F,
 * RGBA16F, B10G11R11F}.comp over RenderCore/extern/spd/ffx_spd.h (the packed path, SpdDownsampleH, with wave operations and
 * SPD_LINEAR_SAMPLER).  Same conventions as sah_hip.h (this header includes it).  Parity unpinned: the reference ships no tests and no
 * images of this pass; what its shaders and Vulkan leave open is fixed below and marked "ABI-defined".
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing, leaves `src` and every cache and epoch of the
 * context untouched, and may be recorded under stream capture.  Hi-Z culling and the draw lists made from it are not part of this library:
 * the reference's culling shader marks every primitive visible (hi_z_culling.comp:147-162).
 */
#ifndef SAH_MIP_CHAIN_H
#define SAH_MIP_CHAIN_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_MIP_CHAIN_MAX_LEVELS 12  /* SPD's limit: imgDst[12] */
#define SAH_MIP_CHAIN_MAX_SOURCE 4096 /* ABI-defined: the largest source extent whose chain SPD's 12 levels cover */

/* MipChainGenerator::fill_mip_chain — "Clear counter" and "Downsample", mip_chain_generator.cpp:63-176.
 *
 * src, dst_levels   dst_levels[i], i < num_dst_levels, are the levels of ONE image: extents max(1, w0 >> i) x max(1, h0 >> i) of level 0's
 *            w0 x h0, one format.  Level 0 may have any extent >= 1 x 1: the reference does not tie it to `src` (DepthCullingPhase passes
 *            src / 2).  Pairs:   src D32_SFLOAT or R32_SFLOAT -> R32_SFLOAT, reduction min;   R16_SFLOAT -> R16_SFLOAT, mean;
 *            R16G16B16A16_SFLOAT -> the same, mean;   B10G11R11_UFLOAT_PACK32 -> the same, mean.
 * Geometry   SpdSetup (ffx_spd.h:327-360) with rect = (0, 0, W, H) of `src`: ceil(W / 64) x ceil(H / 64) workgroups of 256 threads, each
 *            owning a 64 x 64 source tile, and mips = min(floor(log2(float(max(W, H)))), 12).  `mips` comes from the SOURCE extent, not
 *            from num_dst_levels: the kernel makes levels 0 .. max(mips, 1) - 1.
 * Level 0    texel (X, Y), X < 32 * ceil(W / 64), Y < 32 * ceil(H / 64), is ONE sample of `src` (SpdDownsampleMips_0_1_IntrinsicsH,
 *            :956-1002; a sampled value, never a min) at texcoord = fl(fl(tex * inv) + inv) per axis, tex = 2 * (X, Y),
 *            inv = fl(1 / (W, H)); every operator rounded on its own, no fma (ABI-defined).  Sampler: mip_chain_generator.cpp:50-57, LINEAR
 *            with its address modes left at zero, which is REPEAT.  The bilinear rule is the library's (sah_hip.h, sah_texture "tau"):
 *            coordinates u * w - 0.5, an fma chain from +0 over the taps (i, j) (i+1, j) (i, j+1) (i+1, j+1), indices wrapped.  With odd
 *            source extents edge samples therefore blend in the opposite edge, and texels of a tile that lie beyond the image hold
 *            wrapped samples: stores to them are dropped, but they stay live in the workgroup for the levels below.
 *            The sample is converted to half, round to nearest even (ABI-defined: GLSL leaves the rounding of AH4(vec4) open); all later
 *            arithmetic is in half, every operator rounded; fp16 subnormals are kept (reversed-Z depth near the far plane lives there).
 * Reduce     min: min(min(v0, v1), min(v2, v3)); a NaN operand yields the other operand (the library's GLSL rule), -0 orders below +0
 *            (ABI-defined).  mean: (((v0 + v1) + v2) + v3) * 0.25.
 *            Levels 1-5 and 7-11 (SpdReduceQuadH :861-868, :1234): v0 .. v3 = own, right, below, diagonal of the 2 x 2 block of HELD values
 *            of the level above — what the workgroup computed, stored or not.
 *            Level 6 (SpdReduceLoad4H :923-931): (0, 0), (0, 1), (1, 0), (1, 1) — BELOW comes before RIGHT — of STORED level 5.
 * Level 6    only when mips >= 7.  The workgroup that draws numWorkGroups - 1 from the counter goes on alone (:1273-1282).  It sets the
 *            counter back to 0, then all 256 threads read stored level 5 with image-load semantics over 64 x 64 texels (:1209-1237); a
 *            texel outside level 5's extent reads 0 (ABI-defined: undefined in Vulkan without robust image access) — for the min formats
 *            such zeros enter the minimum.  A texel of level 5 that no workgroup stored (level 0 larger than the tiles cover) is read as
 *            the caller left it.
 * Stores     a store outside its level's extent is dropped.  R32 stores the half widened to fp32; B10G11R11 goes through the encoder of
 *            the library's other stores of that format (truncation, negatives to 0, NaN canonical).
 * Missing    the reference binds the image's level 1 to every slot from mipLevels to 11 (:117-124), so a store aimed at a level
 * levels     i >= num_dst_levels lands in LEVEL 1 at the same coordinates.  It happens in the reference's own frame: at 1280 x 720 the Hi-Z
 *            image has 9 levels and SPD writes 10, and after the call texel (0, 0) of level 1 holds the stray last level.  Reproduced.
 *            ABI-defined: the stray store is bounded by the extent the AIMED level would have, max(1, w0 >> i) x max(1, h0 >> i) — under
 *            Vulkan the bound view's extent, level 1's, governs, and more texels of level 1 would be overwritten (4 x 4 at 1280 x 720).
 *            Stray stores of levels >= 6 come after every workgroup's own stores (the counter's release / acquire) and in level order.
 *            Refused (ABI-defined): num_dst_levels == 1 with mips > 1 (no level 1 to take them); num_dst_levels < 6 with mips >= 7 (slot 5
 *            would read level 1); num_dst_levels < mips with mips < 7 and more than one workgroup (no election orders the stray stores
 *            against another workgroup's own).
 * Counter    one uint32 of device memory owned by the context, zeroed on the stream before every launch (the reference's "Clear counter"
 *            pass) and reset by the kernel as well.
 *
 * Planes: aligned to their texel size (2, 4 or 8 bytes) with pitches that are multiples of it.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for any other format pair or for mixed level formats; SAH_ERR_INVALID_ARGUMENT
 * for a NULL pointer, a zero extent, num_dst_levels == 0 or > 12, level extents that are not the Vulkan chain of level 0, a pitch smaller
 * than a row, a misaligned plane, `src` larger than 4096 in either axis, and the three level counts under "Missing levels". */
int sah_mip_chain_generate(sah_ctx* ctx, const sah_plane* src, const sah_plane* dst_levels, uint32_t num_dst_levels);

#ifdef __cplusplus
}
#endif

#endif /* SAH_MIP_CHAIN_H */
