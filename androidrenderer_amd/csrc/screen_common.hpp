// Device helpers shared by the screen-space kernels: taa.hip, taa_upscale.hip, ssao.hip, ssr.hip, motion_blur.hip, sun_shafts.hip, sharpen.hip,
// rt_denoise.hip, rtgi_denoise.hip, exposure.hip and vrsaa.hip.  One definition each; a helper lives here only when every caller gets the
// instructions its own copy gave (DESIGN.md "Device helpers of the screen-space passes": spellings that look alike and compile differently
// stay in their files).  Helpers that read kernel arguments are templates on the argument struct: the passes keep separate structs with
// equal field names.  The names avoid those of texture_sample.hpp (floor_to_int), rt_build_common.hpp (finite3) and lighting_fast.hpp
// (finite_f), which a kernel may include next to this header.
#pragma once
#include "numerics.hpp"
#include "params.hpp"

namespace sah {

constexpr float kScreenInf = __builtin_inff();

// ---- scalars: selects, not fmin / fmax — a NaN takes the second branch
SAH_DEV float clamp01(float a) { return a > 0.0f ? (a < 1.0f ? a : 1.0f) : 0.0f; }
SAH_DEV float max0(float a) { return a > 0.0f ? a : 0.0f; }
SAH_DEV float sel_min(float a, float b) { return a < b ? a : b; }
SAH_DEV float sel_max(float a, float b) { return a > b ? a : b; }
SAH_DEV bool finite_f32(float a) { return __builtin_fabsf(a) < kScreenInf; }
// (bitwise on the compares themselves: no branch, and no warning about & between calls)
SAH_DEV bool all_finite(float a, float b, float c) { return (__builtin_fabsf(a) < kScreenInf) & (__builtin_fabsf(b) < kScreenInf) & (__builtin_fabsf(c) < kScreenInf); }
SAH_DEV bool all_nonneg_finite(float r, float g, float b) { return (r >= 0.0f) & (r < kScreenInf) & (g >= 0.0f) & (g < kScreenInf) & (b >= 0.0f) & (b < kScreenInf); }

SAH_DEV int clampi(int i, int n) { return min(max(i, 0), n - 1); }
// floor(v) as an int, clamped to the int range (a NaN gives the lower bound)
SAH_DEV int floor_i32(float v) { return (int)__builtin_fminf(__builtin_fmaxf(__builtin_floorf(v), -2147483648.0f), 2147483520.0f); }
// the centre of output pixel X in the jittered render raster
SAH_DEV float sample_position(int X, float scale, float jitter) { return ((float)X + 0.5f) * scale - jitter; }

// ---- halfs in dwords and 8-byte texels (x = r | g << 16, y = b | a << 16)
SAH_DEV float half_lo(uint32_t w) { return h2f((uint16_t)(w & 0xffffu)); }
SAH_DEV float half_hi(uint32_t w) { return h2f((uint16_t)(w >> 16)); }
SAH_DEV float texel_channel(uint2 t, int ch) { return h2f((uint16_t)(ch == 0 ? t.x & 0xffffu : ch == 1 ? t.x >> 16 : t.y & 0xffffu)); }
SAH_DEV void unpack_halfs(uint2 t, float (&v)[4]) { v[0] = half_lo(t.x), v[1] = half_hi(t.x), v[2] = half_lo(t.y), v[3] = half_hi(t.y); }
SAH_DEV uint32_t pack_half2(float a, float b) { return (uint32_t)f2h(a) | ((uint32_t)f2h(b) << 16); }

// ---- texel access.  kVec: the address is 8-byte aligned, one 8-byte access; otherwise two dwords (which the compiler may still join)
template <bool kVec> SAH_DEV uint2 load_texel8(const uint8_t* p) {
    if (kVec) return *reinterpret_cast<const uint2*>(p);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    return make_uint2(q[0], q[1]);
}
template <bool kVec> SAH_DEV void store_texel8(uint8_t* p, uint2 v) {
    if (kVec) {
        *reinterpret_cast<uint2*>(p) = v;
    } else {
        reinterpret_cast<uint32_t*>(p)[0] = v.x;
        reinterpret_cast<uint32_t*>(p)[1] = v.y;
    }
}
// I: int or uint32_t, as the kernel counts its pixels (the widening of the index differs)
template <bool kVec, class I> SAH_DEV uint2 load_texel8(const PlaneArg& p, I x, I y) { return load_texel8<kVec>(p.ptr + (size_t)y * p.pitch + (size_t)x * 8); }
template <bool kVec, class I> SAH_DEV void store_texel8(const PlaneArg& p, I x, I y, uint2 v) {
    store_texel8<kVec>(const_cast<uint8_t*>(p.ptr) + (size_t)y * p.pitch + (size_t)x * 8, v);
}
template <class I> SAH_DEV uint32_t load_u32(const PlaneArg& p, I x, I y) { return *reinterpret_cast<const uint32_t*>(p.ptr + (size_t)y * p.pitch + (size_t)x * 4); }
template <class I> SAH_DEV float load_f32(const PlaneArg& p, I x, I y) { return *reinterpret_cast<const float*>(p.ptr + (size_t)y * p.pitch + (size_t)x * 4); }

// (A thread's four-pixel store — two 16-byte stores or eight dwords, the tail of taa.hip, taa_upscale.hip and sharpen.hip — is not here:
// as an inlined function it leaves the kernels another block layout at their end.)

// ---- TAA's luma weight (the resolve and the upscale)
SAH_DEV float taa_luma(float r, float g, float b) { return __builtin_fmaxf((r * 0.2126f + g * 0.7152f) + b * 0.0722f, 0.0f); }

// ---- the view-space surface of a pixel.  A: p20, p21, ipx, ipy, tx, ty (and z_near, m[9] where used)
// view-space x / y of the point at linear depth z under pixel centre cx / cy
template <class A> SAH_DEV float view_x(const A& a, float cx, float z) { return (z * ((cx * a.tx - 1.0f) + a.p20)) * a.ipx; }
template <class A> SAH_DEV float view_y(const A& a, float cy, float z) { return (z * ((cy * a.ty - 1.0f) + a.p21)) * a.ipy; }
// the unit view-space normal of a texel from the bits of its halfs (Centre of sah_ssao.h)
template <class A> SAH_DEV void view_normal(const A& a, uint2 n, float& Nx, float& Ny, float& Nz) {
    const float nx = half_lo(n.x), ny = half_hi(n.x), nz = half_lo(n.y);
    const float vx = (a.m[0] * nx + a.m[3] * ny) + a.m[6] * nz, vy = (a.m[1] * nx + a.m[4] * ny) + a.m[7] * nz, vz = (a.m[2] * nx + a.m[5] * ny) + a.m[8] * nz;
    const float l = __builtin_sqrtf((vx * vx + vy * vy) + vz * vz);
    Nx = vx / l, Ny = vy / l, Nz = vz / l;
}
// "Surface" of sah_rt_denoise.h: false when the pixel has none.  n01, n2: the bits of its normal (x | y << 16, z | w << 16).
template <class A> SAH_DEV bool view_surface(const A& a, int x, int y, float d, uint32_t n01, uint32_t n2, float& z, float P[3], float N[3]) {
    if (!(d > 0.0f)) return false;
    z = a.z_near / d;
    P[0] = view_x(a, (float)x + 0.5f, z), P[1] = view_y(a, (float)y + 0.5f, z), P[2] = -z;
    const float nx = half_lo(n01), ny = half_hi(n01), nz = half_lo(n2);
    const float l = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
    N[0] = nx / l, N[1] = ny / l, N[2] = nz / l;
    return finite_f32(P[0]) && finite_f32(P[1]) && finite_f32(P[2]) && finite_f32(N[0]) && finite_f32(N[1]) && finite_f32(N[2]);
}

// ---- the denoisers' reprojection of pixel (x, y) with view position P and motion vector mv.  A: W, H, djx, djy, iv[12], l2[4], depth_tolerance
struct Reprojection {
    bool valid;          // the previous position lies in the image and in front of the previous camera
    float z_prev, tol;   // the linear depth there as the previous frame saw it, and what a history tap may differ by
    int ix, iy;          // the first bilinear tap (the floor clamped at +-1e9); the others are one texel right / down
    float w4[4];         // the four weights, x first
};
template <class A> SAH_DEV Reprojection reproject(const A& a, int x, int y, uint32_t mv, const float P[3]) {
    Reprojection r;
    const float qx = (((float)x + 0.5f) + half_lo(mv)) + a.djx, qy = (((float)y + 0.5f) + half_hi(mv)) + a.djy;
    r.valid = (qx >= 0.0f) & (qx <= (float)a.W) & (qy >= 0.0f) & (qy <= (float)a.H);
    const float wx = ((a.iv[0] * P[0] + a.iv[3] * P[1]) + a.iv[6] * P[2]) + a.iv[9];
    const float wy = ((a.iv[1] * P[0] + a.iv[4] * P[1]) + a.iv[7] * P[2]) + a.iv[10];
    const float wz = ((a.iv[2] * P[0] + a.iv[5] * P[1]) + a.iv[8] * P[2]) + a.iv[11];
    r.z_prev = -(((a.l2[0] * wx + a.l2[1] * wy) + a.l2[2] * wz) + a.l2[3]);
    r.valid = r.valid && finite_f32(r.z_prev) && r.z_prev > 0.0f;
    r.tol = a.depth_tolerance * r.z_prev;
    const float pxf = qx - 0.5f, pyf = qy - 0.5f;
    const float fx0 = __builtin_floorf(pxf), fy0 = __builtin_floorf(pyf);
    const float fx = pxf - fx0, fy = pyf - fy0;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    r.ix = (int)__builtin_fminf(__builtin_fmaxf(fx0, -1.0e9f), 1.0e9f), r.iy = (int)__builtin_fminf(__builtin_fmaxf(fy0, -1.0e9f), 1.0e9f);
    r.w4[0] = gx * gy, r.w4[1] = fx * gy, r.w4[2] = gx * fy, r.w4[3] = fx * fy;
    return r;
}

}  // namespace sah
