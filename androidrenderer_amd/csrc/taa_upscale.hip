// Temporal upscaling for gfx950 (include/sah_taa_upscale.h): builder-owned arithmetic, restated by tests/taa_upscale_ref.py.
//
// A 256-thread workgroup resolves a 64 x 16 tile of `out`, four adjacent pixels of one row per thread (the shape of taa.hip).  What a tile
// reads of the render planes is a gather: pixel X takes texel i(X) = clamp(floor((X + 0.5) sx - jitter)), and i is monotone in X, so the
// nearest texels of a tile lie between those of its first and its last pixel.  That footprint of `lit` (the raw 8-byte texels) and `depth`,
// one texel of halo on every side, is staged in LDS WITH the clamp applied — cell (r, c) holds texel (clamp(j0 - 1 + r), clamp(i0 - 1 + c)),
// j0 and i0 the first pixel's texel, computed with the very expression the pixels use — so the 3 x 3 stencils read plain neighbours and every
// staged address is a clamped index.  sx, sy <= 1, so the footprint is at most 67 x 19 cells wherever float(X) is exact; a tile whose
// footprint is larger (X, Y beyond 2^24, where float(X) moves in steps) gathers its taps from memory with clamped addresses instead.  The
// motion vector of the chosen tap and the four history texels are gathered through the cache.
//
// The bilinear upsample of `lit` (what a pixel without a usable history stores) is computed only by the pixels that store it; its clamped taps
// lie in the 3 x 3 neighbourhood of (i, j) for every finite u (the header's note), so they are staged cells as well.
//
// kVec: every plane's pointer and pitch are multiples of 16 — texels of lit and history move as 8-byte loads and a thread's four pixels leave
// as two 16-byte stores.  Otherwise every access is a dword.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr int kTuW = 64, kTuH = 16, kTuCols = kTuW + 3, kTuRows = kTuH + 3, kTuPitch = 68;

// The library's bilinear rule at pixel coordinates (post_common.hpp's bilinear<ADDR_CLAMP>): indices and weights of one axis
struct BilinearAxis {
    int a, b;     // the two taps, clamped to [0, n)
    float w0, w1;
};
SAH_DEV BilinearAxis bilinear_axis(float q, int n) {
    const float p = q - 0.5f, p0 = __builtin_floorf(p), f = p - p0;
    const int i = floor_i32(p);
    return {clampi(i, n), clampi(i + 1, n), 1.0f - f, f};
}
// rgb of the four taps (t00, t10, t01, t11: x first) under the weights of the two axes, one fma chain from +0 per channel
SAH_DEV void bilinear_rgb(const BilinearAxis& x, const BilinearAxis& y, uint2 t00, uint2 t10, uint2 t01, uint2 t11, float out[3]) {
    const float w00 = x.w0 * y.w0, w10 = x.w1 * y.w0, w01 = x.w0 * y.w1, w11 = x.w1 * y.w1;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float s = __builtin_fmaf(w00, texel_channel(t00, ch), 0.0f);
        s = __builtin_fmaf(w10, texel_channel(t10, ch), s);
        s = __builtin_fmaf(w01, texel_channel(t01, ch), s);
        out[ch] = __builtin_fmaf(w11, texel_channel(t11, ch), s);
    }
}

// One thread's four pixels.  kStaged: the render texels come from the tile's staged footprint, whose cell (0, 0) is texel (j0 - 1, i0 - 1);
// otherwise from memory.  Either way the texel coordinates asked for may leave the image by one and are clamped.
template <bool kVec, bool kHistory, bool kHdr, bool kStaged>
SAH_DEV void resolve_four(const TaaUpscaleArgs& a, const uint2* s_lit, const float* s_depth, int i0, int j0, int px, int py) {
    const int w = (int)a.w, h = (int)a.h, W = (int)a.W, H = (int)a.H;
    const auto lit_at = [&](int ty, int tx) {
        if (kStaged) return s_lit[(ty - j0 + 1) * kTuPitch + (tx - i0 + 1)];
        return load_texel8<kVec>(a.lit.ptr + (size_t)clampi(ty, h) * a.lit.pitch + (size_t)clampi(tx, w) * 8);
    };
    const auto depth_at = [&](int ty, int tx) {
        if (kStaged) return s_depth[(ty - j0 + 1) * kTuPitch + (tx - i0 + 1)];
        return *reinterpret_cast<const float*>(a.depth.ptr + (size_t)clampi(ty, h) * a.depth.pitch + (size_t)clampi(tx, w) * 4);
    };
    const float wf = (float)a.W, hf = (float)a.H;
    const float uy = sample_position(py, a.sy, a.jy);
    const int j = clampi(floor_i32(uy), h);
    const float ey = (((float)j + 0.5f) - uy) * a.ry;
    uint2 packed[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = min(px + k, W - 1);  // (beyond the image for the last thread of a row: the last pixel again, nothing stored)
        const float ux = sample_position(x, a.sx, a.jx);
        const int i = clampi(floor_i32(ux), w);
        const uint2 centre = lit_at(j, i);
        packed[k] = centre;
        bool stored = false;
        if (kHistory) {
            // Bounds and Motion over the 3 x 3 neighbourhood of (i, j): the nearest tap, the first in tap order among equals, the centre
            // unless a tap is strictly nearer
            float lo[3] = {kScreenInf, kScreenInf, kScreenInf}, hi[3] = {-kScreenInf, -kScreenInf, -kScreenInf};
            float best = depth_at(j, i);
            int bdx = 0, bdy = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const uint2 t = (dx == 0 && dy == 0) ? centre : lit_at(j + dy, i + dx);
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        const float v = texel_channel(t, ch);
                        lo[ch] = __builtin_fminf(lo[ch], v);
                        hi[ch] = __builtin_fmaxf(hi[ch], v);
                    }
                    const float d = depth_at(j + dy, i + dx);
                    const bool nearer = d > best;
                    best = nearer ? d : best;
                    bdx = nearer ? dx : bdx;
                    bdy = nearer ? dy : bdy;
                }
            const uint32_t m = *reinterpret_cast<const uint32_t*>(a.mv.ptr + (size_t)clampi(j + bdy, h) * a.mv.pitch + (size_t)clampi(i + bdx, w) * 4);
            // Position, Validity (output pixels)
            const float qx = ((float)x + 0.5f) + (half_lo(m) + a.djx) * a.rx;
            const float qy = ((float)py + 0.5f) + (half_hi(m) + a.djy) * a.ry;
            bool valid = (qx >= 0.0f) & (qx <= wf) & (qy >= 0.0f) & (qy <= hf);
            // History
            const BilinearAxis bx = bilinear_axis(qx, W), by = bilinear_axis(qy, H);
            const uint8_t* ra = a.history.ptr + (size_t)by.a * a.history.pitch;
            const uint8_t* rb = a.history.ptr + (size_t)by.b * a.history.pitch;
            float hv[3];
            bilinear_rgb(bx, by, load_texel8<kVec>(ra + (size_t)bx.a * 8), load_texel8<kVec>(ra + (size_t)bx.b * 8), load_texel8<kVec>(rb + (size_t)bx.a * 8),
                         load_texel8<kVec>(rb + (size_t)bx.b * 8), hv);
            valid = valid & all_finite(hv[0], hv[1], hv[2]);
            // Clamp
            const float c[3] = {texel_channel(centre, 0), texel_channel(centre, 1), texel_channel(centre, 2)};
            float hc[3];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) hc[ch] = __builtin_fminf(__builtin_fmaxf(hv[ch], lo[ch]), hi[ch]);
            // Confidence, Weight, Blend
            const float ex = (((float)i + 0.5f) - ux) * a.rx;
            const float g = 1.0f - __builtin_fminf(ex * ex + ey * ey, 1.0f);
            const float kb = a.blend * __builtin_fmaxf(g * g, a.min_confidence);
            float wk = kb;
            if (kHdr) {
                const float wc = kb / (1.0f + taa_luma(c[0], c[1], c[2]));
                const float wh = (1.0f - kb) / (1.0f + taa_luma(hc[0], hc[1], hc[2]));
                wk = wc / (wc + wh);
            }
            const float o0 = hc[0] + (c[0] - hc[0]) * wk, o1 = hc[1] + (c[1] - hc[1]) * wk, o2 = hc[2] + (c[2] - hc[2]) * wk;
            stored = valid & all_finite(o0, o1, o2);
            if (stored) {
                packed[k].x = pack_half2(o0, o1);
                packed[k].y = (uint32_t)f2h(o2) | (centre.y & 0xffff0000u);
            }
        }
        if (!stored) {  // Upsample: the taps are texels of the neighbourhood (clamped coordinates within one of (i, j))
            const BilinearAxis bx = bilinear_axis(ux, w), by = bilinear_axis(uy, h);
            float b[3];
            bilinear_rgb(bx, by, lit_at(by.a, bx.a), lit_at(by.a, bx.b), lit_at(by.b, bx.a), lit_at(by.b, bx.b), b);
            if (all_finite(b[0], b[1], b[2])) {
                packed[k].x = pack_half2(b[0], b[1]);
                packed[k].y = (uint32_t)f2h(b[2]) | (centre.y & 0xffff0000u);
            }
        }
    }
    // (the same store ends taa.hip and sharpen.hip: as a shared function it leaves another block layout, see screen_common.hpp)
    uint8_t* row = const_cast<uint8_t*>(a.out.ptr) + (size_t)py * a.out.pitch + (size_t)px * 8;
    if (kVec && px + 3 < W) {
        reinterpret_cast<uint4*>(row)[0] = make_uint4(packed[0].x, packed[0].y, packed[1].x, packed[1].y);
        reinterpret_cast<uint4*>(row)[1] = make_uint4(packed[2].x, packed[2].y, packed[3].x, packed[3].y);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (px + k < W) {
                reinterpret_cast<uint32_t*>(row)[2 * k] = packed[k].x;
                reinterpret_cast<uint32_t*>(row)[2 * k + 1] = packed[k].y;
            }
    }
}

template <bool kVec, bool kHistory, bool kHdr> __global__ void __launch_bounds__(256) k_taa_upscale(TaaUpscaleArgs a) {
    __shared__ __attribute__((aligned(16))) uint2 s_lit[kTuRows * kTuPitch];
    __shared__ __attribute__((aligned(16))) float s_depth[kTuRows * kTuPitch];
    const int tid = (int)threadIdx.x;
    const int w = (int)a.w, h = (int)a.h, W = (int)a.W;
    const int x0 = (int)blockIdx.x * kTuW, y0 = (int)(a.row_begin + blockIdx.y * kTuH);
    const int x1 = min(x0 + kTuW, W) - 1, y1 = min(y0 + kTuH, (int)a.row_end) - 1;  // the tile's last pixel
    // the footprint: texels i0 - 1 .. i1 + 1 by j0 - 1 .. j1 + 1 (0 <= i0 <= i1 < 2^31: the differences do not overflow)
    const int i0 = clampi(floor_i32(sample_position(x0, a.sx, a.jx)), w), i1 = clampi(floor_i32(sample_position(x1, a.sx, a.jx)), w);
    const int j0 = clampi(floor_i32(sample_position(y0, a.sy, a.jy)), h), j1 = clampi(floor_i32(sample_position(y1, a.sy, a.jy)), h);
    const bool staged = (i1 - i0 <= kTuCols - 3) & (j1 - j0 <= kTuRows - 3);  // the same for the whole workgroup
    if (staged) {
        const int cols = i1 - i0 + 3, rows = j1 - j0 + 3;
#pragma unroll
        for (int n = 0; n < (kTuRows * kTuPitch + 255) / 256; n++) {
            const int u = tid + 256 * n;
            const int r = u / kTuPitch, c = u - r * kTuPitch;
            if (r < rows && c < cols) {
                const size_t ty = (size_t)clampi(j0 - 1 + r, h), tx = (size_t)clampi(i0 - 1 + c, w);
                s_lit[r * kTuPitch + c] = load_texel8<kVec>(a.lit.ptr + ty * a.lit.pitch + tx * 8);
                if (kHistory) s_depth[r * kTuPitch + c] = *reinterpret_cast<const float*>(a.depth.ptr + ty * a.depth.pitch + tx * 4);  // (without a history nothing reads the depth)
            }
        }
        __syncthreads();
    }
    const int px = x0 + 4 * (tid & 15), py = y0 + (tid >> 4);
    if (px >= W || py >= (int)a.row_end) return;
    if (staged) resolve_four<kVec, kHistory, kHdr, true>(a, s_lit, s_depth, i0, j0, px, py);
    else resolve_four<kVec, kHistory, kHdr, false>(a, s_lit, s_depth, i0, j0, px, py);
}

hipError_t launch_taa_upscale(const TaaUpscaleArgs& a, bool history, bool hdr_weights, hipStream_t st) {
    if (a.row_end <= a.row_begin) return hipSuccess;
    const dim3 grid((a.W + kTuW - 1) / kTuW, (a.row_end - a.row_begin + kTuH - 1) / kTuH);
    const bool vec = planes_aligned({&a.lit, &a.depth, &a.mv, &a.history, &a.out}, 16);
    void (*kernel)(TaaUpscaleArgs);
    if (!history) kernel = vec ? k_taa_upscale<true, false, false> : k_taa_upscale<false, false, false>;
    else if (hdr_weights) kernel = vec ? k_taa_upscale<true, true, true> : k_taa_upscale<false, true, true>;
    else kernel = vec ? k_taa_upscale<true, true, false> : k_taa_upscale<false, true, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
