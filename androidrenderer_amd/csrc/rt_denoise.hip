// Temporal and edge-aware filter for the ray-traced masks, for gfx950 (include/sah_rt_denoise.h): builder-owned arithmetic, restated by
// tests/rt_denoise_ref.py.
//
// k_rd_temporal: a 256-thread workgroup covers a 64 x 16 tile, four adjacent pixels of one row per thread (the shape of ssao.hip's raw
// kernel).  A pixel's (at most four) history taps are 4- and 2-byte gathers through the cache, one tap where the reprojection lands on a texel's centre; a tap of weight
// 0 or outside the image is not loaded.  kVec: every plane is 16-byte aligned with a pitch that is a multiple of 16 — the thread's four
// samples, depths and motion vectors are one 16-byte load each, its four normals two, its four results one 16-byte and one 8-byte store.
// Otherwise every access is a dword (a half for the lengths).  kOut: passes == 0, the kernel writes `denoised` as well and is the only launch.
//
// k_rd_filter<kPasses>: a 32 x 16 tile; the accumulated value, the linear depth and the unit normal (three halfs) are staged in LDS with
// a halo of 2^kPasses - 1 cells, a cell outside the image or without a surface marked by a NaN depth ("no neighbour"; a real z is
// finite).  Iteration i covers the tile widened by the reach of the iterations after it and writes the other of two value planes in LDS; the
// last covers the tile and writes `denoised`: all iterations in one launch.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr int kRtW = 64, kRtH = 16;  // the temporal kernel's tile
constexpr int kRfW = 32, kRfH = 16;  // the filter kernel's tile: 27.6 KB of LDS with three passes, five workgroups a CU (profiles/rt_denoise.txt has 64 x 16 measured against it)

// One pixel of the temporal pass: the bits of accum_out and of length_out.
template <bool kHistory> SAH_DEV void rd_pixel(const RtDenoiseArgs& a, int x, int y, uint32_t noisy, float d, uint32_t n01, uint32_t n2, uint32_t mv, uint32_t& acc, uint16_t& len) {
    float z, P[3], N[3];
    acc = noisy, len = 0;
    if (!view_surface(a, x, y, d, n01, n2, z, P, N)) return;
    const float s = __builtin_bit_cast(float, noisy);
    const float c = finite_f32(s) ? s : 1.0f;
    acc = __builtin_bit_cast(uint32_t, c), len = 0x3c00u;  // a = c, n = 1
    if (!kHistory) return;
    const int W = (int)a.W, H = (int)a.H;
    const Reprojection rp = reproject(a, x, y, mv, P);
    const bool valid = rp.valid;
    const float z_prev = rp.z_prev, tol = rp.tol;
    float sw = 0.0f, sh = 0.0f, sn = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int u = rp.ix + (t & 1), v = rp.iy + (t >> 1);
        const float w = rp.w4[t];
        if (valid && w > 0.0f && u >= 0 && u < W && v >= 0 && v < H) {
            const float pd = *reinterpret_cast<const float*>(a.prev_depth.ptr + (size_t)v * a.prev_depth.pitch + (size_t)u * 4);
            const float hv = *reinterpret_cast<const float*>(a.history.ptr + (size_t)v * a.history.pitch + (size_t)u * 4);
            const float hl = h2f(*reinterpret_cast<const uint16_t*>(a.hist_len.ptr + (size_t)v * a.hist_len.pitch + (size_t)u * 2));
            const float zt = a.z_near / pd;
            if (pd > 0.0f && __builtin_fabsf(zt - z_prev) <= tol && finite_f32(hv) && finite_f32(hl) && hl >= 1.0f) {
                sw = sw + w;
                sh = sh + w * hv;
                sn = sn + w * hl;
            }
        }
    }
    if (valid && sw > 0.0f) {
        const float h = sh / sw, t = sn / sw + 1.0f;
        const float n = t < a.max_history ? t : a.max_history;
        acc = __builtin_bit_cast(uint32_t, c + (h - c) * (1.0f - 1.0f / n));
        len = f2h(n);
    }
}

template <bool kVec, bool kHistory, bool kOut> __global__ void __launch_bounds__(256) k_rd_temporal(RtDenoiseArgs a) {
    const int tid = (int)threadIdx.x;
    const int W = (int)a.W;
    const int px = (int)blockIdx.x * kRtW + 4 * (tid & 15), py = (int)(a.acc_begin + blockIdx.y * kRtH) + (tid >> 4);
    if (px >= W || py >= (int)a.acc_end) return;
    const uint8_t* srow = a.noisy.ptr + (size_t)py * a.noisy.pitch + (size_t)px * 4;
    const uint8_t* drow = a.depth.ptr + (size_t)py * a.depth.pitch + (size_t)px * 4;
    const uint8_t* nrow = a.normals.ptr + (size_t)py * a.normals.pitch + (size_t)px * 8;
    const uint8_t* mrow = a.mv.ptr + (size_t)py * a.mv.pitch + (size_t)px * 4;
    uint8_t* arow = const_cast<uint8_t*>(a.accum.ptr) + (size_t)py * a.accum.pitch + (size_t)px * 4;
    uint8_t* lrow = const_cast<uint8_t*>(a.length.ptr) + (size_t)py * a.length.pitch + (size_t)px * 2;
    uint8_t* orow = kOut ? const_cast<uint8_t*>(a.out.ptr) + (size_t)py * a.out.pitch + (size_t)px * 4 : nullptr;
    if (kVec && px + 3 < W) {
        const uint4 s = *reinterpret_cast<const uint4*>(srow), m = *reinterpret_cast<const uint4*>(mrow);
        const float4 d = *reinterpret_cast<const float4*>(drow);
        const uint4 na = reinterpret_cast<const uint4*>(nrow)[0], nb = reinterpret_cast<const uint4*>(nrow)[1];
        uint4 o;
        uint16_t l[4];
        rd_pixel<kHistory>(a, px, py, s.x, d.x, na.x, na.y, m.x, o.x, l[0]);
        rd_pixel<kHistory>(a, px + 1, py, s.y, d.y, na.z, na.w, m.y, o.y, l[1]);
        rd_pixel<kHistory>(a, px + 2, py, s.z, d.z, nb.x, nb.y, m.z, o.z, l[2]);
        rd_pixel<kHistory>(a, px + 3, py, s.w, d.w, nb.z, nb.w, m.w, o.w, l[3]);
        *reinterpret_cast<uint4*>(arow) = o;
        *reinterpret_cast<uint2*>(lrow) = make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
        if (kOut) *reinterpret_cast<uint4*>(orow) = o;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (px + k < W) {
                const uint32_t s = reinterpret_cast<const uint32_t*>(srow)[k], m = reinterpret_cast<const uint32_t*>(mrow)[k];
                const float d = reinterpret_cast<const float*>(drow)[k];
                const uint32_t n01 = reinterpret_cast<const uint32_t*>(nrow)[2 * k], n2 = reinterpret_cast<const uint32_t*>(nrow)[2 * k + 1];
                uint32_t o;
                uint16_t l;
                rd_pixel<kHistory>(a, px + k, py, s, d, n01, n2, m, o, l);
                reinterpret_cast<uint32_t*>(arow)[k] = o;
                reinterpret_cast<uint16_t*>(lrow)[k] = l;
                if (kOut) reinterpret_cast<uint32_t*>(orow)[k] = o;
            }
    }
}

// One cell of an iteration of stride S: the plane at v, depths at zs, normals at ns, all of one pitch.
template <int S> SAH_DEV float rd_filter_cell(const float* v, const float* zs, const uint2* ns, int idx, int pitch, float sharp, uint32_t squarings) {
    const float zc = zs[idx], vc = v[idx];
    if (zc != zc) return vc;
    const float gc = sharp / zc;
    const uint2 nc = ns[idx];
    const float cx = half_lo(nc.x), cy = half_hi(nc.x), cz = half_lo(nc.y);
    float wsum = 0.0f, dsum = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            if (dx == 0 && dy == 0) {
                wsum = wsum + 0.25f;
                dsum = dsum + 0.25f * (vc - vc);
                continue;
            }
            const int j = idx + dy * S * pitch + dx * S;
            const float zt = zs[j];
            if (zt == zt) {
                const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
                const float dw = max0(1.0f - __builtin_fabsf(zt - zc) * gc);
                const uint2 nt = ns[j];
                const float ex = half_lo(nt.x), ey = half_hi(nt.x), ez = half_lo(nt.y);
                float e = max0((cx * ex + cy * ey) + cz * ez);
                for (uint32_t q = 0; q < squarings; q++) e = e * e;
                const float w = (k * dw) * e;
                wsum = wsum + w;
                dsum = dsum + w * (v[j] - vc);
            }
        }
    return vc + dsum / wsum;
}

template <int kPasses, int kTW> __global__ void __launch_bounds__(256) k_rd_filter(RtDenoiseArgs a) {
    constexpr int R = (1 << kPasses) - 1;             // the halo
    constexpr int CW = kTW + 2 * R, CH = kRfH + 2 * R;  // the staged cells
    __shared__ float s_v0[CH * CW], s_z[CH * CW];
    __shared__ float s_v1[kPasses > 1 ? CH * CW : 1];
    __shared__ uint2 s_n[CH * CW];
    const int tid = (int)threadIdx.x;
    const int W = (int)a.W;
    const int x0 = (int)blockIdx.x * kTW, y0 = (int)(a.row_begin + blockIdx.y * kRfH);
    for (int i = tid; i < CH * CW; i += 256) {
        const int r = i / CW, c = i - r * CW;
        const int gx = x0 - R + c, gy = y0 - R + r;
        float z = __builtin_nanf(""), v = 0.0f;
        uint2 n = make_uint2(0u, 0u);
        if (gx >= 0 && gx < W && gy >= (int)a.acc_begin && gy < (int)a.acc_end) {  // (rows the temporal kernel wrote: every row a written pixel reaches)
            const float d = *reinterpret_cast<const float*>(a.depth.ptr + (size_t)gy * a.depth.pitch + (size_t)gx * 4);
            const uint32_t* np = reinterpret_cast<const uint32_t*>(a.normals.ptr + (size_t)gy * a.normals.pitch + (size_t)gx * 8);
            v = *reinterpret_cast<const float*>(a.accum.ptr + (size_t)gy * a.accum.pitch + (size_t)gx * 4);
            float zz, P[3], N[3];
            if (view_surface(a, gx, gy, d, np[0], np[1], zz, P, N)) {
                z = zz;
                n = make_uint2(pack_half2(N[0], N[1]), (uint32_t)f2h(N[2]));
            }
        }
        s_z[i] = z, s_v0[i] = v, s_n[i] = n;
    }
    __syncthreads();
    if (kPasses > 1) {  // iteration 0, stride 1, over all but the outermost ring
        constexpr int O = 1, RW = CW - 2 * O, RH = CH - 2 * O;
        for (int i = tid; i < RH * RW; i += 256) {
            const int r = i / RW, c = i - r * RW, idx = (r + O) * CW + c + O;
            s_v1[idx] = rd_filter_cell<1>(s_v0, s_z, s_n, idx, CW, a.depth_sharpness, a.normal_squarings);
        }
        __syncthreads();
    }
    if (kPasses > 2) {  // iteration 1, stride 2
        constexpr int O = 3, RW = CW - 2 * O, RH = CH - 2 * O;
        for (int i = tid; i < RH * RW; i += 256) {
            const int r = i / RW, c = i - r * RW, idx = (r + O) * CW + c + O;
            s_v0[idx] = rd_filter_cell<2>(s_v1, s_z, s_n, idx, CW, a.depth_sharpness, a.normal_squarings);
        }
        __syncthreads();
    }
    const float* last = kPasses == 2 ? s_v1 : s_v0;
#pragma unroll
    for (int i = tid; i < kTW * kRfH; i += 256) {
        const int r = i / kTW, c = i - r * kTW;
        const int gx = x0 + c, gy = y0 + r;
        if (gx < W && gy < (int)a.row_end) {
            const int idx = (r + R) * CW + c + R;
            const float o = rd_filter_cell<1 << (kPasses - 1)>(last, s_z, s_n, idx, CW, a.depth_sharpness, a.normal_squarings);
            *reinterpret_cast<float*>(const_cast<uint8_t*>(a.out.ptr) + (size_t)gy * a.out.pitch + (size_t)gx * 4) = o;
        }
    }
}

hipError_t launch_rt_denoise(const RtDenoiseArgs& a, uint32_t passes, bool history, hipStream_t st) {
    if (a.row_end <= a.row_begin || a.acc_end <= a.acc_begin) return hipSuccess;
    // (planes the flag excuses arrive as null, pitch 0)
    const bool vec = planes_aligned({&a.noisy, &a.depth, &a.normals, &a.mv, &a.prev_depth, &a.history, &a.hist_len, &a.accum, &a.length, &a.out}, 16);
    const bool out = passes == 0;
    void (*temporal)(RtDenoiseArgs);
    if (history) temporal = vec ? (out ? k_rd_temporal<true, true, true> : k_rd_temporal<true, true, false>) : (out ? k_rd_temporal<false, true, true> : k_rd_temporal<false, true, false>);
    else temporal = vec ? (out ? k_rd_temporal<true, false, true> : k_rd_temporal<true, false, false>) : (out ? k_rd_temporal<false, false, true> : k_rd_temporal<false, false, false>);
    const dim3 tgrid((a.W + kRtW - 1) / kRtW, (a.acc_end - a.acc_begin + kRtH - 1) / kRtH);
    hipLaunchKernelGGL(temporal, tgrid, dim3(256), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess || out) return e;
    const dim3 fgrid((a.W + kRfW - 1) / kRfW, (a.row_end - a.row_begin + kRfH - 1) / kRfH);
    void (*filter)(RtDenoiseArgs) = k_rd_filter<1, kRfW>;
    if (passes == 2) filter = k_rd_filter<2, kRfW>;
    if (passes == 3) filter = k_rd_filter<3, kRfW>;
    hipLaunchKernelGGL(filter, fgrid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
