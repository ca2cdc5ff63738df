// The two VRSAA passes for gfx950 (include/sah_vrsaa.h):
//   RenderCore/shaders/vrsaa/contrast_detection.comp:15-68            (host: render/phase/sampling_rate_calculator.cpp:55-76)
//   RenderCore/shaders/vrsaa/generate_shading_rate_image.comp:19-63   (host: sampling_rate_calculator.cpp:32-53, 126-175)
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

// ---- contrast detection --------------------------------------------------------------------------------------------------------------
// A 256-thread workgroup produces a 64 x 16 tile, four adjacent pixels of one row per thread (one 16-byte store).  The taps of pixel p are
// the texels the NEAREST / CLAMP_TO_EDGE sampler returns for texcoord (p + o) / resolution, o in [-1, 1]^2: index map(s) =
// clamp(floor(fl(fl(s / n) * n)), 0, n - 1) per axis, which is s or s - 1 inside the image.  The maps of the tile's 66 columns and 18 rows
// are tabulated once per workgroup (one divide per entry instead of eighteen per pixel), and the tile's footprint is staged in LDS WITH
// the maps applied — cell (r, c) holds texel (map_y(y0 - 1 + r), map_x(x0 - 1 + c)), the edge-replication-at-staging idea of post.hip's bloom
// tiles — so the stencil reads plain neighbours and no tap computes an address.  Every staged address is a clamped index: in bounds by
// construction, whatever the tile's position.  Colour is decoded to luma once per staged texel (sRGB table of the context, copied to LDS).
//
// The 3 x 3 sums keep the shader's nine terms in its order (y outer, x inner, from +0, every operator rounded on its own).  Regrouping them
// into a row pass and a column pass changes roundings — ((a + b) + c) - d - e - f is not (a + b + c) - (d + e + f) in fp32 — so it is not
// done.  Products with a zero weight are dropped for luma only: luma is finite, the running sum starts at +0 and a sum of finite terms is
// never -0 under round-to-nearest, so adding +-0 leaves its bits.  Depth keeps them: inf * 0 = NaN is part of the definition.
constexpr int kCtW = 64, kCtH = 16, kCtCols = kCtW + 2, kCtRows = kCtH + 2, kCtPitch = 68;  // pitch: rows stay 16-byte aligned (ds_read_b128)
constexpr int kCtCells = kCtCols * kCtRows, kCtLoads = (kCtCells + 255) / 256;

SAH_DEV int nearest_clamped(int s, uint32_t n) {
    const float nf = (float)n;
    const float p = ((float)s / nf) * nf;
    const int i = (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf(p), -1.0e9f), 1.0e9f);
    return min(max(i, 0), (int)n - 1);
}

// t[y][x]: the nine taps.  sobel_x[x][y] = {1, 2, 1}[x] * {1, 0, -1}[y], sobel_y[x][y] = {1, 0, -1}[x] * {1, 2, 1}[y] (column-major mat3
// indexed [x][y]: the names are swapped relative to what they measure; the index is followed).
template <bool kKeepZeroWeights> SAH_DEV void sobel(const float t[3][3], float& gx, float& gy) {
    const float a[3] = {1.0f, 2.0f, 1.0f}, b[3] = {1.0f, 0.0f, -1.0f};
    gx = 0.0f;
    gy = 0.0f;
#pragma unroll
    for (int y = 0; y < 3; y++) {
#pragma unroll
        for (int x = 0; x < 3; x++) {
            const float wx = a[x] * b[y], wy = b[x] * a[y];
            if (kKeepZeroWeights || wx != 0.0f) gx = gx + t[y][x] * wx;
            if (kKeepZeroWeights || wy != 0.0f) gy = gy + t[y][x] * wy;
        }
    }
}

__global__ void __launch_bounds__(256) k_vrsaa_contrast(PlaneArg color, PlaneArg depth, PlaneArg out, uint32_t W, uint32_t H, uint32_t row_begin,
                                                         uint32_t row_end, const float* __restrict__ luts, int vec_store) {
    __shared__ __attribute__((aligned(16))) float s_luma[kCtRows * kCtPitch];
    __shared__ __attribute__((aligned(16))) float s_depth[kCtRows * kCtPitch];
    __shared__ float s_lut[256];
    __shared__ int s_xmap[kCtCols], s_ymap[kCtRows];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * kCtW, y0 = (int)(row_begin + blockIdx.y * kCtH);
    s_lut[tid] = luts[tid];
    if (tid < kCtCols) s_xmap[tid] = nearest_clamped(x0 - 1 + tid, W);
    if (tid >= 128 && tid < 128 + kCtRows) s_ymap[tid - 128] = nearest_clamped(y0 - 1 + (tid - 128), H);
    __syncthreads();
    // staging: every load of the thread is issued before its first LDS store
    uint32_t c[kCtLoads];
    float d[kCtLoads];
#pragma unroll
    for (int i = 0; i < kCtLoads; i++) {
        const int k = tid + 256 * i;
        if (k < kCtCells) {
            const int r = k / kCtCols, col = k - r * kCtCols;
            const size_t sy = (size_t)s_ymap[r], sx = (size_t)s_xmap[col];
            c[i] = *reinterpret_cast<const uint32_t*>(color.ptr + sy * color.pitch + sx * 4);
            d[i] = *reinterpret_cast<const float*>(depth.ptr + sy * depth.pitch + sx * 4);
        }
    }
#pragma unroll
    for (int i = 0; i < kCtLoads; i++) {
        const int k = tid + 256 * i;
        if (k < kCtCells) {
            const int r = k / kCtCols, col = k - r * kCtCols;
            // to_luminance (:13) on the sRGB-decoded texel
            const float lr = s_lut[c[i] & 0xffu], lg = s_lut[(c[i] >> 8) & 0xffu], lb = s_lut[(c[i] >> 16) & 0xffu];
            s_luma[r * kCtPitch + col] = (lr * 0.2126f + lg * 0.7152f) + lb * 0.0722f;
            s_depth[r * kCtPitch + col] = d[i];
        }
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    const uint32_t px = (uint32_t)(x0 + 4 * tx), py = (uint32_t)(y0 + ty);
    if (px >= W || py >= row_end) return;
    float l[3][6], z[3][6];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float4 la = *reinterpret_cast<const float4*>(&s_luma[(ty + r) * kCtPitch + 4 * tx]);
        const float2 lb = *reinterpret_cast<const float2*>(&s_luma[(ty + r) * kCtPitch + 4 * tx + 4]);
        const float4 za = *reinterpret_cast<const float4*>(&s_depth[(ty + r) * kCtPitch + 4 * tx]);
        const float2 zb = *reinterpret_cast<const float2*>(&s_depth[(ty + r) * kCtPitch + 4 * tx + 4]);
        l[r][0] = la.x, l[r][1] = la.y, l[r][2] = la.z, l[r][3] = la.w, l[r][4] = lb.x, l[r][5] = lb.y;
        z[r][0] = za.x, z[r][1] = za.y, z[r][2] = za.z, z[r][3] = za.w, z[r][4] = zb.x, z[r][5] = zb.y;
    }
    uint32_t packed[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float tl[3][3], tz[3][3];
#pragma unroll
        for (int y = 0; y < 3; y++)
#pragma unroll
            for (int x = 0; x < 3; x++) tl[y][x] = l[y][k + x], tz[y][x] = z[y][k + x];
        float lx, ly, zx, zy;
        sobel<false>(tl, lx, ly);
        sobel<true>(tz, zx, zy);
        // :62-67: max(luma_gradient * 0.5, depth_gradient); max is maxNum (a NaN depth gradient leaves the luma term, which is never NaN)
        const float ox = __builtin_fmaxf(lx * 0.5f, zx), oy = __builtin_fmaxf(ly * 0.5f, zy);
        packed[k] = pack_half2(ox, oy);
    }
    uint8_t* row = const_cast<uint8_t*>(out.ptr) + (size_t)py * out.pitch + (size_t)px * 4;
    if (vec_store && px + 3 < W) {
        *reinterpret_cast<uint4*>(row) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (px + k < W) *reinterpret_cast<uint32_t*>(row + 4 * k) = packed[k];
    }
}

hipError_t launch_vrsaa_contrast(const PlaneArg& color, const PlaneArg& depth, const PlaneArg& out, uint32_t w, uint32_t h, uint32_t row_begin,
                                 uint32_t row_end, const float* luts, hipStream_t st) {
    if (row_end <= row_begin) return hipSuccess;
    const dim3 grid((w + kCtW - 1) / kCtW, (row_end - row_begin + kCtH - 1) / kCtH);
    const int vec_store = planes_aligned({&out}, 16);
    hipLaunchKernelGGL(k_vrsaa_contrast, grid, dim3(256), 0, st, color, depth, out, w, h, row_begin, row_end, luts, vec_store);
    return hipGetLastError();
}

// ---- shading-rate image --------------------------------------------------------------------------------------------------------------
// A group of G adjacent lanes (a power of two up to a whole wave, chosen from d * d at launch) shares one shading-rate texel: its lanes walk
// the texel's d x d block of the contrast image row by row, lane after lane along x, so a 16 x 16 block is four loads of sixteen-texel row
// segments per lane group and not 256 dependent loads of one thread.  Texels outside the contrast image read 0, and max(m, |0 * 0|) = m for
// m >= +0: the walk covers the in-range part of the block only.  The maximum is maxNum over values that are >= +0 or NaN (|g * g|), from
// +0: NaN never enters, +0 is the only zero, and the maximum of such a set does not depend on the order — so the lanes' partial maxima are
// merged by a butterfly.  Lane 0 of the group then runs the shader's rate search and stores the byte.
__global__ void __launch_bounds__(256) k_vrsaa_shading_rate(PlaneArg contrast, uint32_t cw, uint32_t ch, PlaneArg out, uint32_t sw, uint32_t sh, uint32_t d,
                                                             uint32_t group_shift, uint32_t blocks_x, sah_shading_rate_params prm) {
    const uint32_t G = 1u << group_shift, per_block = 256u >> group_shift;
    const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const uint32_t tx = bx * per_block + (threadIdx.x >> group_shift), ty = by, lane = threadIdx.x & (G - 1);
    float mx = 0.0f, my = 0.0f;
    if (tx < sw) {  // (d * tx, d * ty < 2^31: checked by the entry point)
        const uint32_t bx0 = d * tx, by0 = d * ty;
        const uint32_t ni = bx0 < cw ? min(d, cw - bx0) : 0u, nj = by0 < ch ? min(d, ch - by0) : 0u;
        if (ni && nj) {
            const uint32_t total = ni * nj, qi = G / ni, ri = G - qi * ni;
            uint32_t j = lane / ni, i = lane - j * ni;
            for (uint32_t e = lane; e < total; e += G) {
                const uint32_t t = *reinterpret_cast<const uint32_t*>(contrast.ptr + (size_t)(by0 + j) * contrast.pitch + (size_t)(bx0 + i) * 4);
                const float gx = half_lo(t), gy = half_hi(t);
                mx = __builtin_fmaxf(mx, __builtin_fabsf(gx * gx));
                my = __builtin_fmaxf(my, __builtin_fabsf(gy * gy));
                i += ri;
                j += qi;
                if (i >= ni) i -= ni, j++;
            }
        }
    }
    for (uint32_t o = G >> 1; o > 0; o >>= 1) {  // every lane of the wave takes part (a group never straddles a wave)
        mx = __builtin_fmaxf(mx, __shfl_xor(mx, (int)o));
        my = __builtin_fmaxf(my, __shfl_xor(my, (int)o));
    }
    if (lane != 0 || tx >= sw) return;
    // :39-44
    const float ax = __builtin_fminf(1.25f * __builtin_sqrtf(mx), 1.0f), ay = __builtin_fminf(1.25f * __builtin_sqrtf(my), 1.0f);
    const float R = (float)max(prm.max_rate[0], prm.max_rate[1]);
    const float ox = ax * 1.0f + (1.0f - ax) * R, oy = ay * 1.0f + (1.0f - ay) * R;
    // :46-57: strict <, the first of equal costs stays
    uint32_t best = 0;
    float cost = 1.0f + (2.0f * R) * R;
    for (uint32_t k = 0; k < prm.num_shading_rates; k++) {
        const float dx = (float)prm.rates[k][0] - ox, dy = (float)prm.rates[k][1] - oy;
        const float c = dx * dx + dy * dy;
        if (c < cost) cost = c, best = k;
    }
    const uint32_t rx = prm.rates[best][0], ry = prm.rates[best][1];
    const_cast<uint8_t*>(out.ptr)[(size_t)ty * out.pitch + tx] = (uint8_t)((ry >> 1) | ((rx << 1) & 12u));
}

hipError_t launch_vrsaa_shading_rate(const PlaneArg& contrast, uint32_t cw, uint32_t ch, const PlaneArg& out, uint32_t sw, uint32_t sh, uint32_t d,
                                     const sah_shading_rate_params& params, hipStream_t st) {
    const uint64_t block = (uint64_t)d * d;
    uint32_t shift = 0;
    while (shift < 6 && (1ull << shift) < block) shift++;
    const uint32_t per_block = 256u >> shift, blocks_x = (sw + per_block - 1) / per_block;
    const uint64_t blocks = (uint64_t)blocks_x * sh;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vrsaa_shading_rate, dim3((uint32_t)blocks), dim3(256), 0, st, contrast, cw, ch, out, sw, sh, d, shift, blocks_x, params);
    return hipGetLastError();
}

}  // namespace sah
