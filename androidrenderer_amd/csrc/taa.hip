// Temporal anti-aliasing for gfx950 (include/sah_taa.h): builder-owned arithmetic, restated by tests/taa_ref.py.
//
// A 256-thread workgroup resolves a 64 x 16 tile, four adjacent pixels of one row per thread (the shape of vrsaa.hip's contrast kernel).  The
// tile's footprint of `lit` (the raw 8-byte texels) and `depth`, one texel of halo on every side, is staged in LDS WITH the clamp applied —
// cell (r, c) holds texel (clamp(y0 - 1 + r), clamp(x0 - 1 + c)) — so the 3 x 3 stencils read plain neighbours, and every staged address is
// a clamped index: in bounds whatever the tile's position.  The motion vector of the chosen tap and the four history texels are gathered
// through the cache: one tap per pixel, coherent between neighbours.
//
// kVec: every plane's pointer and pitch are multiples of 16 — the tile's interior is staged with 16-byte loads, the history with 8-byte
// loads, and a thread's four pixels leave as two 16-byte stores.  Otherwise every access is a dword.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr int kTaW = 64, kTaH = 16, kTaCols = kTaW + 2, kTaRows = kTaH + 2, kTaPitch = 68;  // pitch: a thread's six cells are 16-byte aligned
constexpr int kTaLitUnits = kTaW / 2 + 2, kTaDepthUnits = kTaW / 4 + 2;                     // per row: pairs / quads of interior cells + two halo cells

template <bool kVec, bool kHistory, bool kHdr> __global__ void __launch_bounds__(256) k_taa_resolve(TaaArgs a) {
    __shared__ __attribute__((aligned(16))) uint2 s_lit[kTaRows * kTaPitch];
    __shared__ __attribute__((aligned(16))) float s_depth[kTaRows * kTaPitch];
    const int tid = (int)threadIdx.x;
    const int W = (int)a.W, H = (int)a.H;
    const int x0 = (int)blockIdx.x * kTaW, y0 = (int)(a.row_begin + blockIdx.y * kTaH);
    // ---- staging: cell 0 and cell 65 of a row are the halo, cells 1 .. 64 the tile
#pragma unroll
    for (int i = 0; i < (kTaRows * kTaLitUnits + 255) / 256; i++) {
        const int u = tid + 256 * i;
        if (u < kTaRows * kTaLitUnits) {
            const int r = u / kTaLitUnits, j = u - r * kTaLitUnits;
            const uint8_t* row = a.lit.ptr + (size_t)clampi(y0 - 1 + r, H) * a.lit.pitch;
            uint2* dst = &s_lit[r * kTaPitch];
            if (j >= kTaW / 2) {
                const int col = j == kTaW / 2 ? 0 : kTaCols - 1;
                dst[col] = load_texel8<kVec>(row + (size_t)clampi(x0 - 1 + col, W) * 8);
            } else {
                const int gx = x0 + 2 * j;
                if (kVec && gx + 1 < W) {
                    const uint4 v = *reinterpret_cast<const uint4*>(row + (size_t)gx * 8);
                    dst[1 + 2 * j] = make_uint2(v.x, v.y);
                    dst[2 + 2 * j] = make_uint2(v.z, v.w);
                } else {
                    dst[1 + 2 * j] = load_texel8<kVec>(row + (size_t)clampi(gx, W) * 8);
                    dst[2 + 2 * j] = load_texel8<kVec>(row + (size_t)clampi(gx + 1, W) * 8);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < (kTaRows * kTaDepthUnits + 255) / 256; i++) {
        const int u = tid + 256 * i;
        if (kHistory && u < kTaRows * kTaDepthUnits) {  // (without a history nothing reads the depth)
            const int r = u / kTaDepthUnits, j = u - r * kTaDepthUnits;
            const uint8_t* row = a.depth.ptr + (size_t)clampi(y0 - 1 + r, H) * a.depth.pitch;
            float* dst = &s_depth[r * kTaPitch];
            if (j >= kTaW / 4) {
                const int col = j == kTaW / 4 ? 0 : kTaCols - 1;
                dst[col] = *reinterpret_cast<const float*>(row + (size_t)clampi(x0 - 1 + col, W) * 4);
            } else {
                const int gx = x0 + 4 * j;
                if (kVec && gx + 3 < W) {
                    const float4 v = *reinterpret_cast<const float4*>(row + (size_t)gx * 4);
                    dst[1 + 4 * j] = v.x, dst[2 + 4 * j] = v.y, dst[3 + 4 * j] = v.z, dst[4 + 4 * j] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) dst[1 + 4 * j + k] = *reinterpret_cast<const float*>(row + (size_t)clampi(gx + k, W) * 4);
                }
            }
        }
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    const int px = x0 + 4 * tx, py = y0 + ty;
    if (px >= W || py >= (int)a.row_end) return;
    // the thread's 3 x 6 cells; column minima and maxima are shared by the pixels (min / max over a set: any grouping gives the same bits)
    uint2 centre[4];
    float z[3][6], cmin[6][3], cmax[6][3];
    {
        float l[3][6][3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const uint4* src = reinterpret_cast<const uint4*>(&s_lit[(ty + r) * kTaPitch + 4 * tx]);
            const uint4 q0 = src[0], q1 = src[1], q2 = src[2];
            const uint32_t w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
            for (int c = 0; c < 6; c++) {
                l[r][c][0] = half_lo(w[2 * c]), l[r][c][1] = half_hi(w[2 * c]), l[r][c][2] = half_lo(w[2 * c + 1]);
            }
            if (r == 1) {
#pragma unroll
                for (int k = 0; k < 4; k++) centre[k] = make_uint2(w[2 * k + 2], w[2 * k + 3]);
            }
            const float4 za = *reinterpret_cast<const float4*>(&s_depth[(ty + r) * kTaPitch + 4 * tx]);
            const float2 zb = *reinterpret_cast<const float2*>(&s_depth[(ty + r) * kTaPitch + 4 * tx + 4]);
            z[r][0] = za.x, z[r][1] = za.y, z[r][2] = za.z, z[r][3] = za.w, z[r][4] = zb.x, z[r][5] = zb.y;
        }
#pragma unroll
        for (int c = 0; c < 6; c++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                cmin[c][ch] = __builtin_fminf(__builtin_fminf(l[0][c][ch], l[1][c][ch]), l[2][c][ch]);
                cmax[c][ch] = __builtin_fmaxf(__builtin_fmaxf(l[0][c][ch], l[1][c][ch]), l[2][c][ch]);
            }
    }
    const float wf = (float)a.W, hf = (float)a.H;
    uint2 packed[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        packed[k] = centre[k];
        if (!kHistory) continue;
        const int x = px + k;  // (beyond the image for the last thread of a row: clamped addresses, nothing stored)
        // Motion: the nearest tap of the neighbourhood, the first in tap order among equals, the centre unless a tap is strictly nearer
        float best = z[1][k + 1];
        int bdx = 0, bdy = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const float d = z[dy + 1][k + 1 + dx];
                const bool nearer = d > best;
                best = nearer ? d : best;
                bdx = nearer ? dx : bdx;
                bdy = nearer ? dy : bdy;
            }
        const uint32_t m = *reinterpret_cast<const uint32_t*>(a.mv.ptr + (size_t)clampi(py + bdy, H) * a.mv.pitch + (size_t)clampi(x + bdx, W) * 4);
        // Position, Validity
        const float qx = (((float)x + 0.5f) + half_lo(m)) + a.djx, qy = (((float)py + 0.5f) + half_hi(m)) + a.djy;
        bool valid = (qx >= 0.0f) & (qx <= wf) & (qy >= 0.0f) & (qy <= hf);
        // History: bilinear<ADDR_CLAMP> of post_common.hpp at pixel coordinates, rgb only
        const float pxf = qx - 0.5f, pyf = qy - 0.5f;
        const float fx0 = __builtin_floorf(pxf), fy0 = __builtin_floorf(pyf);
        const float fx = pxf - fx0, fy = pyf - fy0;
        const float wx0 = 1.0f - fx, wy0 = 1.0f - fy;
        const int ix = (int)__builtin_fminf(__builtin_fmaxf(fx0, -1.0e9f), 1.0e9f), iy = (int)__builtin_fminf(__builtin_fmaxf(fy0, -1.0e9f), 1.0e9f);
        const size_t xa = (size_t)clampi(ix, W) * 8, xb = (size_t)clampi(ix + 1, W) * 8;
        const uint8_t* ra = a.history.ptr + (size_t)clampi(iy, H) * a.history.pitch;
        const uint8_t* rb = a.history.ptr + (size_t)clampi(iy + 1, H) * a.history.pitch;
        const uint2 t00 = load_texel8<kVec>(ra + xa), t10 = load_texel8<kVec>(ra + xb), t01 = load_texel8<kVec>(rb + xa), t11 = load_texel8<kVec>(rb + xb);
        const float w00 = wx0 * wy0, w10 = fx * wy0, w01 = wx0 * fy, w11 = fx * fy;
        float h[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            float s = __builtin_fmaf(w00, texel_channel(t00, ch), 0.0f);
            s = __builtin_fmaf(w10, texel_channel(t10, ch), s);
            s = __builtin_fmaf(w01, texel_channel(t01, ch), s);
            h[ch] = __builtin_fmaf(w11, texel_channel(t11, ch), s);
        }
        valid = valid & all_finite(h[0], h[1], h[2]);
        // Bounds, Clamp
        const float c[3] = {half_lo(centre[k].x), half_hi(centre[k].x), half_lo(centre[k].y)};
        float hc[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float lo = __builtin_fminf(__builtin_fminf(__builtin_fminf(kScreenInf, cmin[k][ch]), cmin[k + 1][ch]), cmin[k + 2][ch]);
            const float hi = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(-kScreenInf, cmax[k][ch]), cmax[k + 1][ch]), cmax[k + 2][ch]);
            hc[ch] = __builtin_fminf(__builtin_fmaxf(h[ch], lo), hi);
        }
        // Weight, Blend
        float wk = a.blend;
        if (kHdr) {
            const float wc = a.blend / (1.0f + taa_luma(c[0], c[1], c[2]));
            const float wh = (1.0f - a.blend) / (1.0f + taa_luma(hc[0], hc[1], hc[2]));
            wk = wc / (wc + wh);
        }
        const float o0 = hc[0] + (c[0] - hc[0]) * wk, o1 = hc[1] + (c[1] - hc[1]) * wk, o2 = hc[2] + (c[2] - hc[2]) * wk;
        if (valid & all_finite(o0, o1, o2)) {
            packed[k].x = pack_half2(o0, o1);
            packed[k].y = (uint32_t)f2h(o2) | (centre[k].y & 0xffff0000u);
        }
    }
    // (the same store ends taa_upscale.hip and sharpen.hip: as a shared function it leaves another block layout, see screen_common.hpp)
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

hipError_t launch_taa_resolve(const TaaArgs& a, bool history, bool hdr_weights, hipStream_t st) {
    if (a.row_end <= a.row_begin) return hipSuccess;
    const dim3 grid((a.W + kTaW - 1) / kTaW, (a.row_end - a.row_begin + kTaH - 1) / kTaH);
    const bool vec = planes_aligned({&a.lit, &a.depth, &a.mv, &a.history, &a.out}, 16);
    void (*kernel)(TaaArgs);
    if (!history) kernel = vec ? k_taa_resolve<true, false, false> : k_taa_resolve<false, false, false>;
    else if (hdr_weights) kernel = vec ? k_taa_resolve<true, true, true> : k_taa_resolve<false, true, true>;
    else kernel = vec ? k_taa_resolve<true, true, false> : k_taa_resolve<false, true, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
