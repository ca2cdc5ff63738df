// Volumetric sun light for gfx950 (include/sah_sun_shafts.h): builder-owned arithmetic, restated by tests/sun_shafts_ref.py.
//
// A 256-thread workgroup covers 32 x 8 march texels, each of its four waves an 8 x 8 tile, one texel per lane (Lighting's tile shape:
// neighbouring rays walk neighbouring shadow texels, so a wave's four taps of one sample land in a few cache lines).
// ss_texel: the per-texel set-up — the end point, the two inverse products, the four cascade end points and the two divides by the ray
// length — happens once; the sample loop is a product and a sum per coordinate, the cascade selection as compares and selects (no indexed
// register array: no private segment), and Lighting's own shadow_pcf with the format branch hoisted out of the loop by a template
// parameter, so that a sample's four taps issue back to back.  D[k] comes from the kernel arguments with a wave-uniform index: scalar loads.
// A wave leaves the loop at the first k where all its lanes have frac == 0 (frac never grows with k).
// k_ss_march<kFused>: downscale 1 is ONE launch — the thread that marched a texel also composites its pixel from the halfs it has just
// rounded, which are what the stored texel widens to.  Downscale 2 runs the march over the rows of `march` the band needs and then
// k_ss_composite, one pixel per thread, which gathers the four texels and the five depths of the depth-aware bilinear.
#include <hip/hip_runtime.h>

#include "dither.hpp"
#include "launch.hpp"
#include "lighting_common.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr float kSsInv4Pi = 0.07957747f;

namespace {
SAH_DEV uint32_t ss_half(float v) { return v != v ? 0x7E00u : (uint32_t)f2h(v); }
SAH_DEV float ss_sel(uint32_t c, float v0, float v1, float v2, float v3) { return c == 0 ? v0 : (c == 1 ? v1 : (c == 2 ? v2 : v3)); }

// (the planes are 4-byte aligned: texels move as load_texel8<false> / store_texel8<false>, two dwords the compiler joins into one access)
SAH_DEV float ss_depth(const SunShaftsArgs& a, uint32_t x, uint32_t y) {
    const float d = load_f32(a.depth, x, y);
    return d > a.d_min ? d : a.d_min;
}

// Sums of the header: E and V of one ray.  kD16: the map's format, a constant inside shadow_pcf once it is inlined.
template <bool kD16>
SAH_DEV void ss_sums(const SunShaftsArgs& a, float ez, float n, float r, float o, const float (&dl)[4][3], float& E, float& V) {
    CsmArgs csm = a.csm;
    csm.is_d16 = kD16;
    const bool map = a.csm.shadowmap.ptr != nullptr;
    const int steps = (int)a.num_steps;
    E = 0.0f, V = 0.0f;
    for (int k = 0; k < steps; k++) {
        const float kf = (float)k;
        const float frac = clamp01(n - kf);
        if (!wave_any(frac > 0.0f)) break;
        const float t = (kf + o * frac) * r;
        const float zv = ez * t;
        uint32_t cas = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
            if (zv < a.csm.splits[i]) cas = i + 1;
        float vis = 1.0f;
        if (map && frac > 0.0f && cas < a.num_cascades) {
            const float spx = ss_sel(cas, a.a[0][0], a.a[1][0], a.a[2][0], a.a[3][0]) + ss_sel(cas, dl[0][0], dl[1][0], dl[2][0], dl[3][0]) * t;
            const float spy = ss_sel(cas, a.a[0][1], a.a[1][1], a.a[2][1], a.a[3][1]) + ss_sel(cas, dl[0][1], dl[1][1], dl[2][1], dl[3][1]) * t;
            const float spz = ss_sel(cas, a.a[0][2], a.a[1][2], a.a[2][2], a.a[3][2]) + ss_sel(cas, dl[0][2], dl[1][2], dl[2][2], dl[3][2]) * t;
            // inside [0, 1]^3, which a NaN is not: only then does an address follow from the coordinates
            if ((spx >= 0.0f) & (spx <= 1.0f) & (spy >= 0.0f) & (spy <= 1.0f) & (spz >= 0.0f) & (spz <= 1.0f)) {
                float ref = spz - a.depth_bias;
                if (kD16) ref = ref < 0.0f ? 0.0f : (ref > 1.0f ? 1.0f : ref);
                vis = shadow_pcf(csm, spx, spy, cas, ref);
            }
        }
        const float Dk = a.D[k];
        E = E + frac * Dk;
        V = V + (vis * frac) * Dk;
    }
}

// Texel of the header: the march texel that stands for render pixel (x, y), as its four halfs
SAH_DEV uint2 ss_texel(const SunShaftsArgs& a, uint32_t mx, uint32_t my, uint32_t x, uint32_t y) {
    const float d = ss_depth(a, x, y);
    const Fn tx = (Fn((float)x) + Fn(0.5f)) / Fn(a.wf), ty = (Fn((float)y) + Fn(0.5f)) / Fn(a.hf);
    const F4 ndc = {tx * Fn(2.0f) - Fn(1.0f), ty * Fn(2.0f) - Fn(1.0f), Fn(d), Fn(1.0f)};
    const F4 vs = mul44(a.inv_proj, ndc);
    const float ex = (vs.x / vs.w).v, ey = (vs.y / vs.w).v, ez = (vs.z / vs.w).v;
    const float L = __builtin_sqrtf((ex * ex + ey * ey) + ez * ez);
    const F4 B = mul44(a.inv_view, F4{Fn(ex), Fn(ey), Fn(ez), Fn(1.0f)});
    float dl[4][3];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const F4 b = mul44(a.csm.biased[c], B);
        dl[c][0] = (b.x / b.w).v - a.a[c][0];
        dl[c][1] = (b.y / b.w).v - a.a[c][1];
        dl[c][2] = (b.z / b.w).v - a.a[c][2];
    }
    const float n = L / a.step_length, r = a.step_length / L;
    float o = 0.5f;
    if (a.flags & SAH_SUN_SHAFTS_DITHER) o = ((float)(((uint32_t)bayer4x4(mx, my) + a.dither_offset) & 15u) + 0.5f) * 0.0625f;
    float E, V;
    if (a.csm.is_d16) ss_sums<true>(a, ez, n, r, o, dl, E, V);
    else ss_sums<false>(a, ez, n, r, o, dl, E, V);
    const float c = ((ex / L) * a.lv[0] + (ey / L) * a.lv[1]) + (ez / L) * a.lv[2];
    const float q = a.g1 - a.g3 * c;
    const float ph = (a.g2 / (q * __builtin_sqrtf(q))) * kSsInv4Pi;
    const float T = 1.0f - E;
    uint32_t hs[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) hs[ch] = ss_half(E * a.ambient[ch] + (ph * a.sun_color[ch]) * (a.albedo[ch] * V));
    return make_uint2(hs[0] | (hs[1] << 16), hs[2] | (ss_half(T) << 16));
}

// Composite of the header from (S', T') for pixel (x, y); `texel` the march texel's own bits where there is one (downscale 1)
SAH_DEV void ss_write(const SunShaftsArgs& a, uint32_t x, uint32_t y, const float (&st)[4], bool own, uint2 texel) {
    uint2 res;
    if (a.flags & SAH_SUN_SHAFTS_TERM_ONLY) {
        res = own ? texel : make_uint2(ss_half(st[0]) | (ss_half(st[1]) << 16), ss_half(st[2]) | (ss_half(st[3]) << 16));
    } else {
        const uint2 l = load_texel8<false>(a.lit, x, y);
        res = l;
        float lf[4], o[3];
        unpack_halfs(l, lf);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) o[ch] = lf[ch] * st[3] + st[ch];
        const bool identity = (st[3] == 1.0f) & (st[0] == 0.0f) & (st[1] == 0.0f) & (st[2] == 0.0f);
        const bool finite = all_finite(o[0], o[1], o[2]);
        if (!identity && finite) res = make_uint2(pack_half2(o[0], o[1]), (uint32_t)f2h(o[2]) | (l.y & 0xffff0000u));
    }
    store_texel8<false>(a.out, x, y, res);
}
}  // namespace

template <bool kFused> __global__ void __launch_bounds__(256) k_ss_march(SunShaftsArgs a) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t group_y = blockIdx.x / a.groups_x, group_x = blockIdx.x - group_y * a.groups_x;  // (rows folded into grid.x, as k_ssr_trace)
    const uint32_t mx = group_x * 32u + wave * 8u + (lane & 7u), my = a.march_row_begin + group_y * 8u + (lane >> 3);
    if (mx >= a.mw || my >= a.march_row_end) return;
    const uint32_t x = kFused ? mx : mx * a.downscale, y = kFused ? my : my * a.downscale;
    const uint2 texel = ss_texel(a, mx, my, x, y);
    store_texel8<false>(a.march, mx, my, texel);
    if (kFused) {
        float st[4];
        unpack_halfs(texel, st);
        ss_write(a, x, y, st, true, texel);
    }
}

// downscale 2
__global__ void __launch_bounds__(256) k_ss_composite(SunShaftsArgs a) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t group_y = blockIdx.x / a.groups_x, group_x = blockIdx.x - group_y * a.groups_x;
    const uint32_t x = group_x * 32u + wave * 8u + (lane & 7u), y = a.row_begin + group_y * 8u + (lane >> 3);
    if (x >= a.w || y >= a.row_end) return;
    const uint32_t X[2] = {x >> 1, min((x >> 1) + 1u, a.mw - 1u)}, Y[2] = {y >> 1, min((y >> 1) + 1u, a.mh - 1u)};
    const float fx = (x & 1u) ? 0.5f : 0.0f, fy = (y & 1u) ? 0.5f : 0.0f;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float bw[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
    const float z = a.z_near / ss_depth(a, x, y);
    float W[4], t[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t mx = X[j & 1], my = Y[j >> 1];
        const float zj = a.z_near / ss_depth(a, 2u * mx, 2u * my);
        W[j] = bw[j] * (1.0f / (1.0f + (a.depth_sharpness * __builtin_fabsf(z - zj)) / z));
        unpack_halfs(load_texel8<false>(a.march, mx, my), t[j]);
    }
    const float sum = ((W[0] + W[1]) + W[2]) + W[3];
    float st[4];
#pragma unroll
    for (int ch = 0; ch < 4; ch++) st[ch] = (((W[0] * t[0][ch] + W[1] * t[1][ch]) + W[2] * t[2][ch]) + W[3] * t[3][ch]) / sum;
    ss_write(a, x, y, st, false, make_uint2(0u, 0u));
}

hipError_t launch_sun_shafts(const SunShaftsArgs& args, hipStream_t st) {
    if (args.row_end <= args.row_begin) return hipSuccess;
    SunShaftsArgs a = args;
    // w, h < 2^31 and w * h < 2^32 (api_sun_shafts.cpp): the group counts stay below 2^31 however thin the frame
    a.groups_x = (a.mw + 31u) / 32u;
    const uint64_t march_groups = (uint64_t)a.groups_x * ((a.march_row_end - a.march_row_begin + 7u) / 8u);
    if (march_groups > 0x7fffffffull || !march_groups) return hipErrorInvalidConfiguration;
    if (a.downscale == 1) {
        hipLaunchKernelGGL(k_ss_march<true>, dim3((uint32_t)march_groups), dim3(256), 0, st, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_ss_march<false>, dim3((uint32_t)march_groups), dim3(256), 0, st, a);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    a.groups_x = (a.w + 31u) / 32u;
    const uint64_t groups = (uint64_t)a.groups_x * ((a.row_end - a.row_begin + 7u) / 8u);
    if (groups > 0x7fffffffull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_ss_composite, dim3((uint32_t)groups), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
