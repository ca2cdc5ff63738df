// Temporal accumulation and variance-guided filter for the RTGI ray planes, for gfx950 (include/sah_rtgi_denoise.h): builder-owned
// arithmetic, restated by tests/rtgi_denoise_ref.py.  "Surface" and the reprojection are rt_denoise.hip's, shared through
// screen_common.hpp.
//
// k_gd_temporal: a 256-thread workgroup covers a 64 x 8 tile, two adjacent pixels of one row per thread.  kVec: every plane is 16-byte
// aligned with a pitch that is a multiple of 16 — the thread's two rays, irradiances and normals are one 16-byte load each, its depths and
// motion vectors one 8-byte load each, a history tap one 16-byte gather (and an 8-byte one for the moments), accum_out one 16-byte store
// per pixel and moments_out one for the pair.  Otherwise every access is a dword.  A tap of weight 0 or outside the image is not loaded.
// kOut: passes == 0, the kernel writes the two denoised planes as well and is the only launch.
//
// k_gd_filter<kPasses, kTW, kTH>: per cell of the tile and its halo of 2^kPasses - 1 the linear depth (a NaN marks "no neighbour": outside
// the image or the rows the temporal kernel wrote, or no surface), the unit normal as three halfs with the "short history" bit in the
// fourth, and rgb and the variance twice (ping-pong), one LDS array per component: 44 bytes a cell.  Iteration i covers the tile widened
// by the reach of the iterations after it; the last covers the tile and writes the two denoised planes: all iterations in one launch.
// The variance's 3 x 3 mean reads stride-1 neighbours, which lie inside what the iteration before wrote.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr int kGtW = 64, kGtH = 8;   // the temporal kernel's tile
constexpr int kGfW = 16, kGfH = 16;  // the filter kernel's tile: 39.6 KB of LDS with three passes, four workgroups a CU (profiles/rtgi_denoise.txt has 32 x 16 and 32 x 8 measured against it)

SAH_DEV float gd_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// One pixel of the temporal pass.  rb, ri, nrm: the 64 bits of its ray, irradiance and normal.  acc: accum_out's texel, mom: moments_out's;
// orb, oir: the texels of the two denoised planes when passes == 0.
template <bool kVec, bool kHistory>
SAH_DEV void gd_pixel(const RtgiDenoiseArgs& a, int x, int y, uint2 rb, uint2 ri, float d, uint2 nrm, uint32_t mv, float acc[4], float mom[2], uint2& orb, uint2& oir) {
    float z, P[3], N[3];
    acc[0] = acc[1] = acc[2] = acc[3] = 0.0f, mom[0] = mom[1] = 0.0f;
    orb = rb, oir = ri;
    if (!view_surface(a, x, y, d, nrm.x, nrm.y, z, P, N)) return;
    const float dx = half_lo(rb.x), dy = half_hi(rb.x), dz = half_lo(rb.y);
    const float cs = clamp01((dx * N[0] + dy * N[1]) + dz * N[2]);
    float c[5];
    c[0] = half_lo(ri.x) * cs, c[1] = half_hi(ri.x) * cs, c[2] = half_lo(ri.y) * cs;
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = finite_f32(c[k]) ? c[k] : 0.0f;
    c[3] = gd_lum(c[0], c[1], c[2]);
    c[4] = c[3] * c[3];
    float n = 1.0f;
    if (kHistory) {
        const int W = (int)a.W, H = (int)a.H;
        const Reprojection rp = reproject(a, x, y, mv, P);
        const bool valid = rp.valid;
        const float z_prev = rp.z_prev, tol = rp.tol;
        float sw = 0.0f, sn = 0.0f, s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int u = rp.ix + (t & 1), v = rp.iy + (t >> 1);
            const float w = rp.w4[t];
            if (valid && w > 0.0f && u >= 0 && u < W && v >= 0 && v < H) {
                const float pd = *reinterpret_cast<const float*>(a.prev_depth.ptr + (size_t)v * a.prev_depth.pitch + (size_t)u * 4);
                const uint8_t* hp = a.history.ptr + (size_t)v * a.history.pitch + (size_t)u * 16;
                const uint8_t* mp = a.hist_mom.ptr + (size_t)v * a.hist_mom.pitch + (size_t)u * 8;
                float h[5], hn;
                if (kVec) {
                    const float4 hv = *reinterpret_cast<const float4*>(hp);
                    const float2 hm = *reinterpret_cast<const float2*>(mp);
                    h[0] = hv.x, h[1] = hv.y, h[2] = hv.z, hn = hv.w, h[3] = hm.x, h[4] = hm.y;
                } else {
                    const float* hf = reinterpret_cast<const float*>(hp);
                    const float* mf = reinterpret_cast<const float*>(mp);
                    h[0] = hf[0], h[1] = hf[1], h[2] = hf[2], hn = hf[3], h[3] = mf[0], h[4] = mf[1];
                }
                const float zt = a.z_near / pd;
                if (pd > 0.0f && __builtin_fabsf(zt - z_prev) <= tol && finite_f32(hn) && hn >= 1.0f && finite_f32(h[0]) && finite_f32(h[1]) && finite_f32(h[2]) &&
                    finite_f32(h[3]) && finite_f32(h[4])) {
                    sw = sw + w;
                    sn = sn + w * hn;
#pragma unroll
                    for (int k = 0; k < 5; k++) s[k] = s[k] + w * h[k];
                }
            }
        }
        if (valid && sw > 0.0f) {
            const float t = sn / sw + 1.0f;
            n = t < a.max_history ? t : a.max_history;
            const float kk = 1.0f - 1.0f / n;
#pragma unroll
            for (int k = 0; k < 5; k++) c[k] = c[k] + (s[k] / sw - c[k]) * kk;
        }
    }
    acc[0] = c[0], acc[1] = c[1], acc[2] = c[2], acc[3] = n, mom[0] = c[3], mom[1] = c[4];
    orb = make_uint2(pack_half2(N[0], N[1]), (uint32_t)f2h(N[2]) | (rb.y & 0xffff0000u));
    oir = make_uint2(pack_half2(c[0], c[1]), (uint32_t)f2h(c[2]));
}

template <bool kVec, bool kHistory, bool kOut> __global__ void __launch_bounds__(256) k_gd_temporal(RtgiDenoiseArgs a) {
    const int tid = (int)threadIdx.x;
    const int W = (int)a.W;
    const int px = (int)blockIdx.x * kGtW + 2 * (tid & 31), py = (int)(a.acc_begin + blockIdx.y * kGtH) + (tid >> 5);
    if (px >= W || py >= (int)a.acc_end) return;
    const uint8_t* rrow = a.rays.ptr + (size_t)py * a.rays.pitch + (size_t)px * 8;
    const uint8_t* irow = a.irr.ptr + (size_t)py * a.irr.pitch + (size_t)px * 8;
    const uint8_t* drow = a.depth.ptr + (size_t)py * a.depth.pitch + (size_t)px * 4;
    const uint8_t* nrow = a.normals.ptr + (size_t)py * a.normals.pitch + (size_t)px * 8;
    const uint8_t* mrow = a.mv.ptr + (size_t)py * a.mv.pitch + (size_t)px * 4;
    uint8_t* arow = const_cast<uint8_t*>(a.accum.ptr) + (size_t)py * a.accum.pitch + (size_t)px * 16;
    uint8_t* qrow = const_cast<uint8_t*>(a.moments.ptr) + (size_t)py * a.moments.pitch + (size_t)px * 8;
    uint8_t* orow = kOut ? const_cast<uint8_t*>(a.out_rays.ptr) + (size_t)py * a.out_rays.pitch + (size_t)px * 8 : nullptr;
    uint8_t* erow = kOut ? const_cast<uint8_t*>(a.out_irr.ptr) + (size_t)py * a.out_irr.pitch + (size_t)px * 8 : nullptr;
    if (kVec && px + 1 < W) {
        const uint4 rb = *reinterpret_cast<const uint4*>(rrow), ri = *reinterpret_cast<const uint4*>(irow), nn = *reinterpret_cast<const uint4*>(nrow);
        const float2 d = *reinterpret_cast<const float2*>(drow);
        const uint2 m = *reinterpret_cast<const uint2*>(mrow);
        float a0[4], a1[4], m0[2], m1[2];
        uint2 ob0, oi0, ob1, oi1;
        gd_pixel<true, kHistory>(a, px, py, make_uint2(rb.x, rb.y), make_uint2(ri.x, ri.y), d.x, make_uint2(nn.x, nn.y), m.x, a0, m0, ob0, oi0);
        gd_pixel<true, kHistory>(a, px + 1, py, make_uint2(rb.z, rb.w), make_uint2(ri.z, ri.w), d.y, make_uint2(nn.z, nn.w), m.y, a1, m1, ob1, oi1);
        reinterpret_cast<float4*>(arow)[0] = make_float4(a0[0], a0[1], a0[2], a0[3]);
        reinterpret_cast<float4*>(arow)[1] = make_float4(a1[0], a1[1], a1[2], a1[3]);
        *reinterpret_cast<float4*>(qrow) = make_float4(m0[0], m0[1], m1[0], m1[1]);
        if (kOut) {
            *reinterpret_cast<uint4*>(orow) = make_uint4(ob0.x, ob0.y, ob1.x, ob1.y);
            *reinterpret_cast<uint4*>(erow) = make_uint4(oi0.x, oi0.y, oi1.x, oi1.y);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2; k++)
            if (px + k < W) {
                const uint32_t* rp = reinterpret_cast<const uint32_t*>(rrow) + 2 * k;
                const uint32_t* ip = reinterpret_cast<const uint32_t*>(irow) + 2 * k;
                const uint32_t* np = reinterpret_cast<const uint32_t*>(nrow) + 2 * k;
                const float d = reinterpret_cast<const float*>(drow)[k];
                const uint32_t m = reinterpret_cast<const uint32_t*>(mrow)[k];
                float ac[4], mo[2];
                uint2 ob, oi;
                gd_pixel<false, kHistory>(a, px + k, py, make_uint2(rp[0], rp[1]), make_uint2(ip[0], ip[1]), d, make_uint2(np[0], np[1]), m, ac, mo, ob, oi);
                float* ap = reinterpret_cast<float*>(arow) + 4 * k;
                ap[0] = ac[0], ap[1] = ac[1], ap[2] = ac[2], ap[3] = ac[3];
                float* qp = reinterpret_cast<float*>(qrow) + 2 * k;
                qp[0] = mo[0], qp[1] = mo[1];
                if (kOut) {
                    uint32_t* op = reinterpret_cast<uint32_t*>(orow) + 2 * k;
                    uint32_t* ep = reinterpret_cast<uint32_t*>(erow) + 2 * k;
                    op[0] = ob.x, op[1] = ob.y, ep[0] = oi.x, ep[1] = oi.y;
                }
            }
    }
}

struct GdCells {  // one generation of the filtered pair in LDS
    float *r, *g, *b, *q;
};

// One cell of an iteration of stride S: depths at zs, normals (and the short-history bit) at ns, all of one pitch.  out: r, g, b, variance.
template <int S> SAH_DEV void gd_filter_cell(const RtgiDenoiseArgs& a, const GdCells& v, const float* zs, const uint2* ns, int idx, int pitch, float out[4]) {
    const float zc = zs[idx];
    const float vc[3] = {v.r[idx], v.g[idx], v.b[idx]};
    const float qc = v.q[idx];
    out[0] = vc[0], out[1] = vc[1], out[2] = vc[2], out[3] = qc;
    if (zc != zc) return;
    const float gc = a.depth_sharpness / zc;
    const uint2 nc = ns[idx];
    const float cx = half_lo(nc.x), cy = half_hi(nc.x), cz = half_lo(nc.y);
    const bool use_lum = a.luminance_sigma != 0.0f && !(nc.y >> 16);
    const float lc = gd_lum(vc[0], vc[1], vc[2]);
    float den = 1.0f;
    if (use_lum) {
        float gs = 0.0f, ks = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int j = idx + dy * pitch + dx;
                if (zs[j] == zs[j]) {
                    const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
                    gs = gs + k * v.q[j];
                    ks = ks + k;
                }
            }
        den = a.luminance_sigma * __builtin_sqrtf(gs / ks) + a.luminance_floor;
    }
    float wsum = 0.0f, qsum = 0.0f, dsum[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            if (dx == 0 && dy == 0) {
                wsum = wsum + 0.25f;
#pragma unroll
                for (int k = 0; k < 3; k++) dsum[k] = dsum[k] + 0.25f * (vc[k] - vc[k]);
                qsum = qsum + (0.25f * 0.25f) * qc;
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
                for (uint32_t q = 0; q < a.normal_squarings; q++) e = e * e;
                const float vt[3] = {v.r[j], v.g[j], v.b[j]};
                float w = (k * dw) * e;
                if (use_lum) w = w * max0(1.0f - __builtin_fabsf(gd_lum(vt[0], vt[1], vt[2]) - lc) / den);
                wsum = wsum + w;
#pragma unroll
                for (int c = 0; c < 3; c++) dsum[c] = dsum[c] + w * (vt[c] - vc[c]);
                qsum = qsum + (w * w) * v.q[j];
            }
        }
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = vc[k] + dsum[k] / wsum;
    out[3] = qsum / (wsum * wsum);
}

template <int kPasses, int kTW, int kTH> __global__ void __launch_bounds__(256) k_gd_filter(RtgiDenoiseArgs a) {
    constexpr int R = (1 << kPasses) - 1;           // the halo
    constexpr int CW = kTW + 2 * R, CH = kTH + 2 * R;  // the staged cells
    constexpr int C = CH * CW, C1 = kPasses > 1 ? C : 1;
    static_assert(C * 28 + C1 * 16 <= 64 * 1024, "the staged cells fit the LDS a workgroup may declare");
    __shared__ float s_z[C], s_r0[C], s_g0[C], s_b0[C], s_q0[C];
    __shared__ float s_r1[C1], s_g1[C1], s_b1[C1], s_q1[C1];
    __shared__ uint2 s_n[C];
    const GdCells v0{s_r0, s_g0, s_b0, s_q0}, v1{s_r1, s_g1, s_b1, s_q1};
    const int tid = (int)threadIdx.x;
    const int W = (int)a.W;
    const int x0 = (int)blockIdx.x * kTW, y0 = (int)(a.row_begin + blockIdx.y * kTH);
    const bool acc16 = (((uintptr_t)a.accum.ptr | a.accum.pitch) & 15u) == 0, mom8 = (((uintptr_t)a.moments.ptr | a.moments.pitch) & 7u) == 0;
    for (int i = tid; i < C; i += 256) {
        const int r = i / CW, c = i - r * CW;
        const int gx = x0 - R + c, gy = y0 - R + r;
        float z = __builtin_nanf(""), v[3] = {0.0f, 0.0f, 0.0f}, q = 0.0f;
        uint2 n = make_uint2(0u, 0u);
        if (gx >= 0 && gx < W && gy >= (int)a.acc_begin && gy < (int)a.acc_end) {  // (rows the temporal kernel wrote: every row a written pixel reaches)
            const float d = *reinterpret_cast<const float*>(a.depth.ptr + (size_t)gy * a.depth.pitch + (size_t)gx * 4);
            const uint32_t* np = reinterpret_cast<const uint32_t*>(a.normals.ptr + (size_t)gy * a.normals.pitch + (size_t)gx * 8);
            float zz, P[3], N[3];
            if (view_surface(a, gx, gy, d, np[0], np[1], zz, P, N)) {
                const uint8_t* ap = a.accum.ptr + (size_t)gy * a.accum.pitch + (size_t)gx * 16;
                const uint8_t* mp = a.moments.ptr + (size_t)gy * a.moments.pitch + (size_t)gx * 8;
                float4 ac;
                float2 mo;
                if (acc16) ac = *reinterpret_cast<const float4*>(ap);
                else ac = make_float4(reinterpret_cast<const float*>(ap)[0], reinterpret_cast<const float*>(ap)[1], reinterpret_cast<const float*>(ap)[2], reinterpret_cast<const float*>(ap)[3]);
                if (mom8) mo = *reinterpret_cast<const float2*>(mp);
                else mo = make_float2(reinterpret_cast<const float*>(mp)[0], reinterpret_cast<const float*>(mp)[1]);
                z = zz;
                v[0] = ac.x, v[1] = ac.y, v[2] = ac.z;
                q = max0(mo.y - mo.x * mo.x);
                n = make_uint2(pack_half2(N[0], N[1]), (uint32_t)f2h(N[2]) | (ac.w < a.min_history ? 0x10000u : 0u));
            }
        }
        s_z[i] = z, s_r0[i] = v[0], s_g0[i] = v[1], s_b0[i] = v[2], s_q0[i] = q, s_n[i] = n;
    }
    __syncthreads();
    if (kPasses > 1) {  // iteration 0, stride 1, over all but the outermost ring
        constexpr int O = 1, RW = CW - 2 * O, RH = CH - 2 * O;
        for (int i = tid; i < RH * RW; i += 256) {
            const int r = i / RW, c = i - r * RW, idx = (r + O) * CW + c + O;
            float o[4];
            gd_filter_cell<1>(a, v0, s_z, s_n, idx, CW, o);
            s_r1[idx] = o[0], s_g1[idx] = o[1], s_b1[idx] = o[2], s_q1[idx] = o[3];
        }
        __syncthreads();
    }
    if (kPasses > 2) {  // iteration 1, stride 2
        constexpr int O = 3, RW = CW - 2 * O, RH = CH - 2 * O;
        for (int i = tid; i < RH * RW; i += 256) {
            const int r = i / RW, c = i - r * RW, idx = (r + O) * CW + c + O;
            float o[4];
            gd_filter_cell<2>(a, v1, s_z, s_n, idx, CW, o);
            s_r0[idx] = o[0], s_g0[idx] = o[1], s_b0[idx] = o[2], s_q0[idx] = o[3];
        }
        __syncthreads();
    }
    const GdCells& last = kPasses == 2 ? v1 : v0;
    const bool out8 = (((uintptr_t)a.out_rays.ptr | a.out_rays.pitch | (uintptr_t)a.out_irr.ptr | a.out_irr.pitch) & 7u) == 0;
    for (int i = tid; i < kTW * kTH; i += 256) {
        const int r = i / kTW, c = i - r * kTW;
        const int gx = x0 + c, gy = y0 + r;
        if (gx < W && gy < (int)a.row_end) {
            const int idx = (r + R) * CW + c + R;
            const uint32_t* rp = reinterpret_cast<const uint32_t*>(a.rays.ptr + (size_t)gy * a.rays.pitch + (size_t)gx * 8);
            uint2 ob, oi;
            if (s_z[idx] == s_z[idx]) {
                float o[4];
                gd_filter_cell<1 << (kPasses - 1)>(a, last, s_z, s_n, idx, CW, o);
                const uint2 n = s_n[idx];
                ob = make_uint2(n.x, (n.y & 0xffffu) | (rp[1] & 0xffff0000u));
                oi = make_uint2(pack_half2(o[0], o[1]), (uint32_t)f2h(o[2]));
            } else {  // no surface: the 64 bits of both inputs
                const uint32_t* ip = reinterpret_cast<const uint32_t*>(a.irr.ptr + (size_t)gy * a.irr.pitch + (size_t)gx * 8);
                ob = make_uint2(rp[0], rp[1]), oi = make_uint2(ip[0], ip[1]);
            }
            uint8_t* op = const_cast<uint8_t*>(a.out_rays.ptr) + (size_t)gy * a.out_rays.pitch + (size_t)gx * 8;
            uint8_t* ep = const_cast<uint8_t*>(a.out_irr.ptr) + (size_t)gy * a.out_irr.pitch + (size_t)gx * 8;
            if (out8) {
                *reinterpret_cast<uint2*>(op) = ob, *reinterpret_cast<uint2*>(ep) = oi;
            } else {
                reinterpret_cast<uint32_t*>(op)[0] = ob.x, reinterpret_cast<uint32_t*>(op)[1] = ob.y;
                reinterpret_cast<uint32_t*>(ep)[0] = oi.x, reinterpret_cast<uint32_t*>(ep)[1] = oi.y;
            }
        }
    }
}

hipError_t launch_rtgi_denoise(const RtgiDenoiseArgs& a, uint32_t passes, bool history, hipStream_t st) {
    if (a.row_end <= a.row_begin || a.acc_end <= a.acc_begin) return hipSuccess;
    // (planes the flag excuses arrive as null, pitch 0)
    const bool vec = planes_aligned({&a.rays, &a.irr, &a.depth, &a.normals, &a.mv, &a.prev_depth, &a.history, &a.hist_mom, &a.accum, &a.moments, &a.out_rays, &a.out_irr}, 16);
    const bool out = passes == 0;
    void (*temporal)(RtgiDenoiseArgs);
    if (history) temporal = vec ? (out ? k_gd_temporal<true, true, true> : k_gd_temporal<true, true, false>) : (out ? k_gd_temporal<false, true, true> : k_gd_temporal<false, true, false>);
    else temporal = vec ? (out ? k_gd_temporal<true, false, true> : k_gd_temporal<true, false, false>) : (out ? k_gd_temporal<false, false, true> : k_gd_temporal<false, false, false>);
    const dim3 tgrid((a.W + kGtW - 1) / kGtW, (a.acc_end - a.acc_begin + kGtH - 1) / kGtH);
    hipLaunchKernelGGL(temporal, tgrid, dim3(256), 0, st, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess || out) return e;
    const dim3 fgrid((a.W + kGfW - 1) / kGfW, (a.row_end - a.row_begin + kGfH - 1) / kGfH);
    void (*filter)(RtgiDenoiseArgs) = k_gd_filter<1, kGfW, kGfH>;
    if (passes == 2) filter = k_gd_filter<2, kGfW, kGfH>;
    if (passes == 3) filter = k_gd_filter<3, kGfW, kGfH>;
    hipLaunchKernelGGL(filter, fgrid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
