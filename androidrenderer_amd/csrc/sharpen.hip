// Contrast-adaptive sharpening for gfx950 (include/sah_sharpen.h): builder-owned arithmetic, restated by tests/sharpen_ref.py.
//
// A 256-thread workgroup sharpens a 64 x 16 tile, four adjacent pixels of one row per thread (the shape of taa.hip).  What is staged in LDS
// is not the raw texel but its COMPRESSED form — three fp32 channels and the CLEAN flag, 16 bytes a cell — so that the three divisions of
// the range compression are paid once per texel and not once per tap: a thread loads and compresses its own four texels (and keeps their
// raw bits in registers for the alpha and the pass-through rule), and 160 of the threads one texel more of the halo: the row above, the
// row below, the column to the left and the one to the right.  The corners are not needed and not staged.  Every staged address is a
// clamped index — cell (r, c) holds texel (clamp(y0 - 1 + r), clamp(x0 - 1 + c)) — so it is in bounds whatever the tile's position, and
// the stencil reads plain neighbours.  Coordinates are unsigned: no tile of an image below 2^31 texels a side overflows them.
//
// kVec: every pointer and pitch is a multiple of 16 — a thread's four texels arrive as two 16-byte loads and leave as two 16-byte stores,
// a halo texel as one 8-byte load.  Otherwise every access is a dword.  kDenoise: SAH_SHARPEN_DENOISE, compiled in or out.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr uint32_t kShW = 64, kShH = 16, kShCols = kShW + 2, kShRows = kShH + 2;

namespace {

SAH_DEV uint32_t sh_minu(uint32_t a, uint32_t b) { return a < b ? a : b; }

// Compress: the texel (x = r | g << 16, y = b | a << 16) as t.rgb and, in w, the bit pattern 1 where it is CLEAN and 0 where it is not
SAH_DEV float4 sh_compress(uint2 raw, float k) {
    const float r = half_lo(raw.x), g = half_hi(raw.x), b = half_lo(raw.y);
    const bool clean = all_finite(r, g, b) & !(r < 0.0f) & !(g < 0.0f) & !(b < 0.0f);
    const float cr = r * k, cg = g * k, cb = b * k;
    const float d = 1.0f + sel_max(sel_max(cr, cg), cb);
    return make_float4(cr / d, cg / d, cb / d, __builtin_bit_cast(float, clean ? 1u : 0u));
}

SAH_DEV float sh_channel(const float4& v, int ch) { return ch == 0 ? v.x : (ch == 1 ? v.y : v.z); }
SAH_DEV float sh_luma(const float4& p) { return (p.x * 0.5f + p.y) + p.z * 0.5f; }

template <bool kVec, bool kDenoise> __global__ void __launch_bounds__(256) k_sharpen(SharpenArgs a) {
    __shared__ __attribute__((aligned(16))) float4 s_t[kShRows * kShCols];
    const uint32_t tid = threadIdx.x;
    const uint32_t W = a.W, H = a.H;
    const uint32_t tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const uint32_t x0 = tile_x * kShW, y0 = a.row_begin + tile_y * kShH;
    // Scale
    float k = a.pre_scale;
    if (a.exposure) {
        const float kp = a.pre_scale * a.exposure->exposure;
        if (kp >= 0x1p-20f && kp <= 0x1p+20f) k = kp;  // (a NaN and the infinities fail)
    }
    // ---- staging: the thread's own four texels, cells (ty + 1, 4 tx + 1 ..)
    const uint32_t tx = tid & 15u, ty = tid >> 4;
    const uint32_t px = x0 + 4u * tx, py = y0 + ty;
    uint2 centre[4];
    {
        const uint8_t* row = a.scene.ptr + (size_t)sh_minu(py, H - 1u) * a.scene.pitch;
        if (kVec && px + 3u < W) {
            const uint4 v0 = reinterpret_cast<const uint4*>(row + (size_t)px * 8)[0], v1 = reinterpret_cast<const uint4*>(row + (size_t)px * 8)[1];
            centre[0] = make_uint2(v0.x, v0.y), centre[1] = make_uint2(v0.z, v0.w), centre[2] = make_uint2(v1.x, v1.y), centre[3] = make_uint2(v1.z, v1.w);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) centre[j] = load_texel8<kVec>(row + (size_t)sh_minu(px + j, W - 1u) * 8);
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) s_t[(ty + 1u) * kShCols + 4u * tx + 1u + j] = sh_compress(centre[j], k);
    }
    // ---- the halo: threads 0 .. 63 the row above, 64 .. 127 the row below, 128 .. 143 the column to the left, 144 .. 159 the one to the right
    if (tid < 160u) {
        uint32_t r, c;
        if (tid < 128u) {
            r = tid < 64u ? 0u : kShRows - 1u, c = 1u + (tid & 63u);
        } else {
            r = 1u + (tid & 15u), c = tid < 144u ? 0u : kShCols - 1u;
        }
        const uint32_t gy = sh_minu((y0 + r ? y0 + r : 1u) - 1u, H - 1u), gx = sh_minu((x0 + c ? x0 + c : 1u) - 1u, W - 1u);
        s_t[r * kShCols + c] = sh_compress(load_texel8<kVec>(a.scene.ptr + (size_t)gy * a.scene.pitch + (size_t)gx * 8), k);
    }
    __syncthreads();
    if (px >= W || py >= a.row_end) return;
    float4 up[4], mid[6], down[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) up[j] = s_t[ty * kShCols + 4u * tx + 1u + j], down[j] = s_t[(ty + 2u) * kShCols + 4u * tx + 1u + j];
#pragma unroll
    for (uint32_t j = 0; j < 6; j++) mid[j] = s_t[(ty + 1u) * kShCols + 4u * tx + j];
    uint2 packed[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float4 B = up[j], D = mid[j], E = mid[j + 1], F = mid[j + 2], Hh = down[j];
        const bool eligible = (__builtin_bit_cast(uint32_t, B.w) & __builtin_bit_cast(uint32_t, D.w) & __builtin_bit_cast(uint32_t, E.w) &
                               __builtin_bit_cast(uint32_t, F.w) & __builtin_bit_cast(uint32_t, Hh.w)) != 0u;
        // Limiter
        float lobe = 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float b = sh_channel(B, ch), d = sh_channel(D, ch), e = sh_channel(E, ch), f = sh_channel(F, ch), h = sh_channel(Hh, ch);
            const float mn4 = sel_min(sel_min(sel_min(b, d), f), h), mx4 = sel_max(sel_max(sel_max(b, d), f), h);
            const float hit_min = mx4 > 0.0f ? sel_min(mn4, e) / (4.0f * mx4) : 0.0f;
            const float hit_max = (1.0f - sel_max(mx4, e)) / (4.0f * mn4 - 4.0f);
            const float lobe_c = sel_max(-hit_min, hit_max);
            lobe = ch == 0 ? lobe_c : sel_max(lobe, lobe_c);
        }
        lobe = sel_max(-0.1875f, sel_min(lobe, 0.0f)) * a.sharpness;
        // Noise
        if (kDenoise) {
            const float lb = sh_luma(B), ld = sh_luma(D), le = sh_luma(E), lf = sh_luma(F), lh = sh_luma(Hh);
            const float nz = ((lb + ld) + (lf + lh)) * 0.25f - le;
            const float range = sel_max(sel_max(sel_max(sel_max(lb, ld), le), lf), lh) - sel_min(sel_min(sel_min(sel_min(lb, ld), le), lf), lh);
            const float q = range > 0.0f ? sel_min(__builtin_fabsf(nz) / range, 1.0f) : 0.0f;
            lobe = lobe * (1.0f - q * 0.5f);
        }
        // Resolve
        const float den = 4.0f * lobe + 1.0f;
        float s[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float b = sh_channel(B, ch), d = sh_channel(D, ch), e = sh_channel(E, ch), f = sh_channel(F, ch), h = sh_channel(Hh, ch);
            s[ch] = sel_min(sel_max((lobe * ((b + d) + (f + h)) + e) / den, 0.0f), 1.0f);
        }
        // Expand, Store
        const float rest = 1.0f - sel_min(sel_max(sel_max(s[0], s[1]), s[2]), 1.0f - 0x1p-17f);
        const float o0 = sel_min((s[0] / rest) / k, 65504.0f), o1 = sel_min((s[1] / rest) / k, 65504.0f), o2 = sel_min((s[2] / rest) / k, 65504.0f);
        packed[j] = centre[j];
        if (eligible) {
            packed[j].x = pack_half2(o0, o1);
            packed[j].y = (uint32_t)f2h(o2) | (centre[j].y & 0xffff0000u);
        }
    }
    // (the same store ends taa.hip and taa_upscale.hip: as a shared function it leaves another block layout, see screen_common.hpp)
    uint8_t* row = const_cast<uint8_t*>(a.out.ptr) + (size_t)py * a.out.pitch + (size_t)px * 8;
    if (kVec && px + 3u < W) {
        reinterpret_cast<uint4*>(row)[0] = make_uint4(packed[0].x, packed[0].y, packed[1].x, packed[1].y);
        reinterpret_cast<uint4*>(row)[1] = make_uint4(packed[2].x, packed[2].y, packed[3].x, packed[3].y);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            if (px + j < W) {
                reinterpret_cast<uint32_t*>(row)[2 * j] = packed[j].x;
                reinterpret_cast<uint32_t*>(row)[2 * j + 1] = packed[j].y;
            }
    }
}

}  // namespace

hipError_t launch_sharpen(const SharpenArgs& in, bool denoise, hipStream_t st) {
    if (in.row_end <= in.row_begin) return hipSuccess;
    SharpenArgs a = in;
    a.tiles_x = (a.W + kShW - 1) / kShW;
    const dim3 grid(a.tiles_x * ((a.row_end - a.row_begin + kShH - 1) / kShH));  // one dimension: no limit of 65535 tile rows (W * H < 2^32: fits)
    const bool vec = planes_aligned({&a.scene, &a.out}, 16);
    void (*kernel)(SharpenArgs);
    if (denoise) kernel = vec ? k_sharpen<true, true> : k_sharpen<false, true>;
    else kernel = vec ? k_sharpen<true, false> : k_sharpen<false, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
