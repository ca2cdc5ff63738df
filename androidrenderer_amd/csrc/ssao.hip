// Screen-space ambient occlusion for gfx950 (include/sah_ssao.h): builder-owned arithmetic, restated by tests/ssao_ref.py.
//
// k_ssao_raw: a 256-thread workgroup covers a 64 x 16 tile, four adjacent pixels of one row per thread (the shape of taa.hip).  The
// rotated offsets e(k, x & 3, y & 3) are formed once per workgroup into LDS — 256 float2, laid out [k][rotation] so that the (at most four)
// rotations a wave reads for one tap and one of its four pixels are neighbours: broadcast reads, no bank conflict.  A pixel's 16 taps are
// 4-byte gathers of depth through the cache, as the history taps of taa.hip are: the sampling radius is bounded by max_radius_pixels, not
// by anything LDS could hold, and that bound is what keeps a wave's taps inside a few dozen L2-resident rows.  kVec: depth, normals and
// the target are 16-byte aligned with pitches that are multiples of 16 — the thread's four depths are one 16-byte load, its four normals
// two, its four results one 16-byte store.  Otherwise every access is a dword.
//
// k_ssao_blur<kPasses>: a 32 x 16 tile; raw AO and linear depth are staged in LDS with a halo of kPasses texels, a cell outside the image
// or without a surface marked by a NaN depth ("no neighbour"; a real z = z_near / depth with depth > 0 and z_near finite and positive is
// never NaN).  With two passes the first covers tile + 1 into LDS and the second the tile into ao_out: both in one launch.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr int kSrW = 64, kSrH = 16;  // the raw kernel's tile
constexpr int kSbW = 32, kSbH = 16;  // the blur kernel's tile

__constant__ float kSsaoOffsets[SAH_SSAO_TAPS][2] = SAH_SSAO_OFFSETS;
__constant__ float kSsaoRotations[16][2] = SAH_SSAO_ROTATIONS;

// One pixel of the raw pass.  d: its depth; n01, n2: the bits of its normal (x | y << 16, z | w << 16); j4 = 4 * (y & 3), kx = x & 3.
SAH_DEV float ssao_pixel(const SsaoArgs& a, const float2* s_e, int x, int y, float d, uint32_t n01, uint32_t n2) {
    if (!(d > 0.0f)) return 1.0f;
    const float wf = (float)a.W, hf = (float)a.H;
    const float z = a.z_near / d;
    const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
    const float px = view_x(a, cx, z), py = view_y(a, cy, z), pz = -z;
    float Nx, Ny, Nz;
    view_normal(a, make_uint2(n01, n2), Nx, Ny, Nz);
    if (!(finite_f32(px) && finite_f32(py) && finite_f32(pz) && finite_f32(Nx) && finite_f32(Ny) && finite_f32(Nz))) return 1.0f;
    const float t = a.rs / z;
    const float r_px = t > 1.0f ? (t < a.max_radius_pixels ? t : a.max_radius_pixels) : 1.0f;
    const float R = (r_px * z) / a.sx;
    const float RR = R * R;
    const int rot = (x & 3) + 4 * (y & 3);
    float sum = 0.0f;
    int n = 0;
#pragma unroll
    for (int k = 0; k < SAH_SSAO_TAPS; k++) {
        const float2 e = s_e[k * 16 + rot];
        const float fx = cx + e.x * r_px, fy = cy + e.y * r_px;
        const bool inside = (fx >= 0.0f) & (fx < wf) & (fy >= 0.0f) & (fy < hf);
        const int ix = inside ? (int)__builtin_floorf(fx) : 0, iy = inside ? (int)__builtin_floorf(fy) : 0;  // (0, 0) is a texel of every image
        const float dt = *reinterpret_cast<const float*>(a.depth.ptr + (size_t)iy * a.depth.pitch + (size_t)ix * 4);
        bool use = inside & !((ix == x) & (iy == y)) & (dt > 0.0f);
        const float zt = a.z_near / dt;
        const float sx = view_x(a, (float)ix + 0.5f, zt), sy = view_y(a, (float)iy + 0.5f, zt);
        const float dx = sx - px, dy = sy - py, dz = -zt - pz;
        const float vv = (dx * dx + dy * dy) + dz * dz;
        use = use & (vv > 0.0f) & (vv < kScreenInf);
        const float ndotd = ((Nx * dx + Ny * dy) + Nz * dz) / __builtin_sqrtf(vv);
        const float o = max0(ndotd - a.threshold) * clamp01(1.0f - vv / RR);
        sum = use ? sum + o : sum;
        n += use ? 1 : 0;
    }
    if (n == 0) return 1.0f;
    const float fade = clamp01((a.fade_to - z) / a.fade_span);
    const float unclamped = ((sum / (float)n) * a.shadow_multiplier) * fade;
    const float obs = unclamped < a.shadow_clamp ? unclamped : a.shadow_clamp;
    const float occ = 1.0f - obs;
    return occ * __builtin_sqrtf(occ);
}

template <bool kVec> __global__ void __launch_bounds__(256) k_ssao_raw(SsaoArgs a) {
    __shared__ float2 s_e[SAH_SSAO_TAPS * 16];
    const int tid = (int)threadIdx.x;
    {
        const int k = tid >> 4, j = tid & 15;
        const float sx = kSsaoOffsets[k][0], sy = kSsaoOffsets[k][1], c = kSsaoRotations[j][0], sn = kSsaoRotations[j][1];
        s_e[tid] = make_float2(sx * c - sy * sn, sx * sn + sy * c);
    }
    __syncthreads();
    const int W = (int)a.W;
    const int px = (int)blockIdx.x * kSrW + 4 * (tid & 15), py = (int)(a.raw_begin + blockIdx.y * kSrH) + (tid >> 4);
    if (px >= W || py >= (int)a.raw_end) return;
    const uint8_t* drow = a.depth.ptr + (size_t)py * a.depth.pitch + (size_t)px * 4;
    const uint8_t* nrow = a.normals.ptr + (size_t)py * a.normals.pitch + (size_t)px * 8;
    uint8_t* orow = const_cast<uint8_t*>(a.raw.ptr) + (size_t)py * a.raw.pitch + (size_t)px * 4;
    if (kVec && px + 3 < W) {
        const float4 d = *reinterpret_cast<const float4*>(drow);
        const uint4 na = reinterpret_cast<const uint4*>(nrow)[0], nb = reinterpret_cast<const uint4*>(nrow)[1];
        float4 o;
        o.x = ssao_pixel(a, s_e, px, py, d.x, na.x, na.y);
        o.y = ssao_pixel(a, s_e, px + 1, py, d.y, na.z, na.w);
        o.z = ssao_pixel(a, s_e, px + 2, py, d.z, nb.x, nb.y);
        o.w = ssao_pixel(a, s_e, px + 3, py, d.w, nb.z, nb.w);
        *reinterpret_cast<float4*>(orow) = o;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (px + k < W) {
                const float d = reinterpret_cast<const float*>(drow)[k];
                const uint32_t n01 = reinterpret_cast<const uint32_t*>(nrow)[2 * k], n2 = reinterpret_cast<const uint32_t*>(nrow)[2 * k + 1];
                reinterpret_cast<float*>(orow)[k] = ssao_pixel(a, s_e, px + k, py, d, n01, n2);
            }
    }
}

// One cell of a blur pass: the plane at av[ai], its depths at zv[zi]; neighbours one cell left / right and one row (of either pitch) up / down.
SAH_DEV float blur_cell(const float* av, int ai, int apitch, const float* zv, int zi, int zpitch, float sharp) {
    const float zc = zv[zi];
    if (zc != zc) return 1.0f;
    float num = av[ai], den = 1.0f;
    const int zo[4] = {-1, 1, -zpitch, zpitch}, ao[4] = {-1, 1, -apitch, apitch};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float zn = zv[zi + zo[i]];
        if (zn == zn) {
            const float w = max0(1.0f - (__builtin_fabsf(zn - zc) / zc) * sharp);
            num = num + w * av[ai + ao[i]];
            den = den + w;
        }
    }
    return num / den;
}

template <int kPasses> __global__ void __launch_bounds__(256) k_ssao_blur(SsaoArgs a) {
    constexpr int CW = kSbW + 2 * kPasses, CH = kSbH + 2 * kPasses;  // the staged cells
    constexpr int BW = CW - 2, BH = CH - 2;                          // the first pass's cells (two passes)
    __shared__ float s_a[CH * CW], s_z[CH * CW];
    __shared__ float s_b[kPasses == 2 ? BH * BW : 1];
    const int tid = (int)threadIdx.x;
    const int W = (int)a.W, H = (int)a.H;
    const int x0 = (int)blockIdx.x * kSbW, y0 = (int)(a.row_begin + blockIdx.y * kSbH);
    for (int i = tid; i < CH * CW; i += 256) {
        const int r = i / CW, c = i - r * CW;
        const int gx = x0 - kPasses + c, gy = y0 - kPasses + r;
        float z = __builtin_nanf(""), v = 1.0f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const float d = *reinterpret_cast<const float*>(a.depth.ptr + (size_t)gy * a.depth.pitch + (size_t)gx * 4);
            if (d > 0.0f) {
                z = a.z_near / d;
                if (gy >= (int)a.raw_begin && gy < (int)a.raw_end) v = *reinterpret_cast<const float*>(a.raw.ptr + (size_t)gy * a.raw.pitch + (size_t)gx * 4);
            }
        }
        s_z[i] = z, s_a[i] = v;
    }
    __syncthreads();
    if (kPasses == 2) {
        for (int i = tid; i < BH * BW; i += 256) {
            const int r = i / BW, c = i - r * BW;
            s_b[i] = blur_cell(s_a, (r + 1) * CW + c + 1, CW, s_z, (r + 1) * CW + c + 1, CW, a.edge_sharpness);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = tid; i < kSbW * kSbH; i += 256) {
        const int r = i / kSbW, c = i - r * kSbW;
        const int gx = x0 + c, gy = y0 + r;
        if (gx < W && gy < (int)a.row_end) {
            const int zi = (r + kPasses) * CW + c + kPasses;
            const float o = kPasses == 2 ? blur_cell(s_b, (r + 1) * BW + c + 1, BW, s_z, zi, CW, a.edge_sharpness) : blur_cell(s_a, zi, CW, s_z, zi, CW, a.edge_sharpness);
            *reinterpret_cast<float*>(const_cast<uint8_t*>(a.out.ptr) + (size_t)gy * a.out.pitch + (size_t)gx * 4) = o;
        }
    }
}

hipError_t launch_ssao(const SsaoArgs& a, uint32_t blur_passes, hipStream_t st) {
    if (a.row_end <= a.row_begin || a.raw_end <= a.raw_begin) return hipSuccess;
    const bool vec = planes_aligned({&a.depth, &a.normals, &a.raw}, 16);
    const dim3 raw_grid((a.W + kSrW - 1) / kSrW, (a.raw_end - a.raw_begin + kSrH - 1) / kSrH);
    hipLaunchKernelGGL(vec ? k_ssao_raw<true> : k_ssao_raw<false>, raw_grid, dim3(256), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess || blur_passes == 0) return e;
    const dim3 blur_grid((a.W + kSbW - 1) / kSbW, (a.row_end - a.row_begin + kSbH - 1) / kSbH);
    hipLaunchKernelGGL(blur_passes == 2 ? k_ssao_blur<2> : k_ssao_blur<1>, blur_grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
