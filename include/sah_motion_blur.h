/* sah_motion_blur.h — camera motion blur: the scene blurred along the motion vectors the library already produces for sah_taa_resolve,
 * sah_taa_upscale and the denoisers.  The reference has no counterpart: its frame has "Other postprocessing // TODO" where it would go
 * (scene_renderer.cpp:417-419).  This pass is builder-owned, like sah_ssr, sah_sharpen and sah_exposure_*: its arithmetic is fixed below
 * ("ABI-defined"), restated in numpy by tests/motion_blur_ref.py and pinned bit for bit by tests/golden/motion_blur_*.npz.  Parity unpinned.
 * Off by default everywhere: nothing in the library, in include/sah_host.hpp or in androidrenderer_amd/frame.py runs it unless the caller
 * asks.  Its place is after the anti-aliasing and the sharpening and before the exposure: upscale / resolve -> sharpen -> motion blur ->
 * exposure -> bloom -> tonemap.  The filter is the tile-max / neighbour-max reconstruction of McGuire et al. ("A Reconstruction Filter for
 * Plausible Motion Blur", I3D 2012) in rational form.  It blurs the camera's motion only (the vectors carry no per-object motion: the
 * reference has none), is not part of sah_chain_*, and gathers at full resolution.  Same conventions as sah_hip.h (this header includes it).
 *
 * The call runs on the context's stream, does no host synchronisation, allocates nothing, leaves its inputs and every cache and epoch of
 * the context untouched, and may be recorded under stream capture.
 */
#ifndef SAH_MOTION_BLUR_H
#define SAH_MOTION_BLUR_H

#include "sah_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAH_MOTION_BLUR_DITHER 1u /* the taps of pixel (X, Y) are shifted by (b - 7.5) / 16 of a tap spacing, b sah_ssr.h's 4 x 4 matrix at [Y & 3][X & 3] */

/* 44 bytes, host memory, read during the call.  z_near is a field and not a sah_view_data*: it is the only thing of the view the pass
 * reads (the jitters travel in the parameters, as in sah_taa_upscale_params), so a caller behind sah_taa_upscale, which has no view at
 * hand, needs no 1 KB structure for one float. */
typedef struct sah_motion_blur_params {
    float shutter;             /* fraction of the frame interval the shutter is open, in (0, 1]; default 0.5 */
    float max_blur_pixels;     /* cap on a scaled vector's length in render pixels, in (0, 32]; default 32.  The shutter is centred, so a tap lies
                                  at most 16 render pixels, one tile, from its pixel: a 3 x 3 tile neighbourhood holds every mover that reaches it */
    float min_velocity_pixels; /* a pixel whose neighbour velocity is shorter passes through, >= 0 and finite; default 0.5 */
    uint32_t sample_count;     /* taps per pixel, even, 2..32; default 12 */
    float depth_extent;        /* softness of the foreground / background classification in view-space units, finite and > 0; default 1 */
    float z_near;              /* sah_view_data::z_near of the frame, finite and > 0; default 0.1 */
    float jitter[2];           /* this frame's, in render pixels (sah_view_data::jitter); default 0 */
    float previous_jitter[2];  /* default 0 */
    uint32_t flags;            /* SAH_MOTION_BLUR_*; default 0 */
} sah_motion_blur_params;
#define SAH_MOTION_BLUR_DEFAULT_SHUTTER 0.5f
#define SAH_MOTION_BLUR_DEFAULT_MAX_BLUR_PIXELS 32.0f
#define SAH_MOTION_BLUR_DEFAULT_MIN_VELOCITY_PIXELS 0.5f
#define SAH_MOTION_BLUR_DEFAULT_SAMPLE_COUNT 12u
#define SAH_MOTION_BLUR_DEFAULT_DEPTH_EXTENT 1.0f
#define SAH_MOTION_BLUR_DEFAULT_Z_NEAR 0.1f
#define SAH_MOTION_BLUR_DEFAULT_JITTER 0.0f
#define SAH_MOTION_BLUR_DEFAULT_FLAGS 0u
#define SAH_MOTION_BLUR_TILE 16u /* the side of a tile of the render raster */

/* scene, out: R16G16B16A16_SFLOAT, W x H (the output resolution).  depth (D32_SFLOAT, reversed Z) and motion_vectors (R16G16_SFLOAT in
 * render pixels, mv = previous position - pixel centre, as sah_motion_vectors_render writes it): w x h (the render resolution), W >= w and
 * H >= h; the two ratios may differ, equal extents are the common case.  tiles: R16G16_SFLOAT, ceil(w / 16) x ceil(h / 16), caller-owned
 * scratch written by the call.  Every width and height < 2^31, w * h and W * H < 2^32.
 *
 * In fp32, every operator rounded on its own (no contraction anywhere), IEEE division and square root.  All of it is ABI-defined.
 * clamp01(a) = a > 0 ? (a < 1 ? a : 1) : 0 (sah_ssr.h's: a NaN gives 0).  The host forms, with IEEE operations, sx = float(w) / float(W),
 * sy = float(h) / float(H), rx = float(W) / float(w), ry = float(H) / float(h), dj = previous_jitter - jitter and nf = float(sample_count).
 * Steps are given for x; y is likewise.
 * Velocity   of a pair of halfs m (a texel of motion_vectors, or an entry of tiles): a.x = (float(m.x) + dj.x) * shutter;
 *            l2 = a.x * a.x + a.y * a.y; unless l2 < inf (a NaN fails) a = (0, 0) and l2 = 0: a non-finite velocity counts as zero.
 *            l = sqrt(l2); when l > max_blur_pixels: s = max_blur_pixels / l, v = (a.x * s, a.y * s) and the speed |v| is max_blur_pixels
 *            itself; otherwise v = a and |v| = l.  Adding dj takes the jitter out, so under a static camera, whose vectors are
 *            jitter - previous_jitter rounded to halfs, every velocity is zero or a rounding error far below any sensible min_velocity_pixels.
 * Key        of a pair: (l2, the pair's 32 bits x | y << 16), ordered by l2 first (the unclamped one) and by the bit pattern as an
 *            unsigned number second.  It is a total order, so a greatest key does not depend on the order of a reduction.
 * Tile       tiles[ty][tx] = the RAW pair with the greatest key among the texels of motion_vectors in [16 tx, 16 tx + 16) x [16 ty,
 *            16 ty + 16) that lie inside the image.  A selection, not arithmetic: the halfs are stored exactly.  A tile whose every
 *            velocity is zero therefore stores the pair with the greatest bit pattern among its texels — (0, 0) when the vectors are all
 *            zero — and NOT an unconditional (0, 0): the Velocity of a stored (0, 0) is dj * shutter, which a jittered static camera would
 *            then blur along; the selected pair's Velocity is zero, as it must be.
 * Sample     u.x = (float(X) + 0.5) * sx - jitter.x and Nearest i = clamp(int(floor(u.x)), 0, w - 1), both exactly as sah_taa_upscale.h:
 *            output pixel (X, Y) sits at u in the render raster, on render texel (i, j), in tile (i >> 4, j >> 4).
 * Neighbour  vn, |vn| = the Velocity of the pair with the greatest key among the 3 x 3 tiles around the pixel's tile, their coordinates
 *            clamped to the tile grid (a tile counted twice changes no greatest key).
 * Surface    of render texel (i, j) with depth d: z = z_near / d when d > 0, and z = 2^100 when !(d > 0) (no surface) or when
 *            !(z < 2^100): a large finite depth, so no inf - inf arises.
 * Clean      a texel of scene is clean when each of its rgb halfs is >= 0 and < inf (sah_sharpen's rule: -0 is clean, a NaN is not).
 * Own        c = rgb of scene[Y][X]; vp, |vp| = Velocity of motion_vectors[j][i]; zp = Surface of (i, j).
 * Taps       dith = (float(b) - 7.5) * 0.0625 under SAH_MOTION_BLUR_DITHER, b = the matrix 0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5
 *            at [Y & 3][X & 3], otherwise 0.  For k = 0 .. sample_count - 1, each from its index and never by accumulation:
 *            t = ((float(k) + 0.5) + dith) / nf - 0.5; e.x = vn.x * t; p.x = u.x + e.x.  The tap has weight 0 unless 0 <= p.x < float(w)
 *            and 0 <= p.y < float(h) (a NaN fails); its render texel is (floor(p.x), floor(p.y)).  q.x = p.x * rx; weight 0 unless
 *            0 <= q.x < float(W) and 0 <= q.y < float(H); its scene texel s is scene[floor(q.y)][floor(q.x)]; weight 0 unless s is clean.
 *            (Each floor is also held to the last texel of its image, which matters only where float(w) rounds up: some w > 2^24.)
 * Weight     vs, |vs| = Velocity and zs = Surface of the tap's render texel.  d = sqrt(e.x * e.x + e.y * e.y), the distance between tap
 *            and pixel.  z grows with distance here (McGuire's is negative), so the tap is in front when zs < zp:
 *            f = clamp01(1 - (zs - zp) / depth_extent) (1 for a tap in front), g = clamp01(1 - (zp - zs) / depth_extent) (1 for one behind).
 *            cone(s) = clamp01(1 - d / s).  cyl(s) = (y * y) * (3 - 2 * y) with e0 = 0.95 * s, e1 = 1.05 * s,
 *            y = clamp01((e1 - d) / (e1 - e0)): 1 - smoothstep(e0, e1, d) as a clamped cubic, no pow.
 *            wk = (f * cone(|vs|) + g * cone(|vp|)) + (2 * cyl(|vs|)) * cyl(|vp|).
 *            A speed s of 0 gives cone = cyl = 0, without a fault and without a branch: d / 0 is inf or NaN, (e1 - d) / 0 is -inf or NaN,
 *            and clamp01 sends both to 0.  Every wk is finite and >= 0.
 * Result     From sw = 0 and acc = (0, 0, 0), for k ascending over the taps of non-zero weight: sw = sw + wk,
 *            acc.c = acc.c + wk * (float(s.c) - c.c).  r.c = acc.c / sw; o.c = c.c + r.c.  Channel c stores half(o.c), round to nearest
 *            even, where r.c != 0, and scene's 16 bits where r.c == 0 (so a constant image is a fixed point bit for bit whatever the
 *            vectors, -0 included).  Alpha is always scene's 16 bits.
 * The pixel PASSES THROUGH — `out` gets the four halfs of scene[Y][X] bit for bit — when |vn| < min_velocity_pixels, when scene[Y][X] is
 * not clean, when sw == 0 (every tap carries weight 0), or when a channel of o is not finite.
 *
 * Every plane 4-byte aligned with a pitch that is a multiple of 4 (the rules of sah_taa_resolve); when scene, out, depth and
 * motion_vectors all have pointers and pitches that are multiples of 16 the pass takes a path with 8- and 16-byte accesses.  The bytes
 * written are the same on either path.  The library allocates nothing.
 *
 * Rows [row_begin, row_end) of `out` are written ((0, 0) = all rows), and a pixel's value does not depend on the row window.  With
 * j0 = j(row_begin), j1 = j(row_end - 1) (Nearest) and T0 = max(j0 / 16 - 1, 0), T1 = min(j1 / 16 + 1, ceil(h / 16) - 1), a non-empty
 * band writes rows T0 .. T1 of tiles in full, reads rows 16 T0 .. min(16 T1 + 15, h - 1) of motion_vectors for them, rows [row_begin,
 * row_end) of scene for the pixels' own texels, and, for the taps, rows j0 - 16 .. j1 + 16 of depth and motion_vectors and rows
 * floor((j0 - 16) ry) .. floor((j1 + 17) ry) of scene, clamped to the images.  An empty band writes and launches nothing.
 *
 * Before anything is launched: SAH_ERR_UNSUPPORTED_FORMAT for a plane of another format; SAH_ERR_INVALID_ARGUMENT for a NULL pointer, a
 * zero extent, scene and out not sharing one extent, depth and motion_vectors not sharing one extent, tiles other than ceil(w / 16) x
 * ceil(h / 16), w > W or h > H (downscaling), 2^32 texels or more, a pitch smaller than a row, a misaligned plane, row_begin > row_end or
 * row_end > H, shutter outside (0, 1], max_blur_pixels outside (0, 32], a min_velocity_pixels that is not finite and >= 0, a sample_count
 * that is odd or outside 2..32, a depth_extent or z_near that is not finite and > 0, a jitter that is not finite, a NaN in any parameter,
 * an undefined flag bit, the byte range of `out` overlapping that of an input or of tiles, and tiles overlapping an input. */
int sah_motion_blur(sah_ctx* ctx, const sah_plane* scene, const sah_plane* depth, const sah_plane* motion_vectors, const sah_plane* tiles,
                    const sah_plane* out, const sah_motion_blur_params* params, uint32_t row_begin, uint32_t row_end);

#ifdef __cplusplus
}
#endif

#endif /* SAH_MOTION_BLUR_H */
