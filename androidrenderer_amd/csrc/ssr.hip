// Screen-space reflections for gfx950 (include/sah_ssr.h): builder-owned arithmetic, restated by tests/ssr_ref.py.
//
// k_ssr_trace: a 256-thread workgroup covers 32 x 8 pixels, each of its four waves an 8 x 8 pixel block (lane & 7, lane >> 3), one pixel per
// lane.  The march is a data-dependent loop whose trip count is the slowest lane's: the rays of a compact block leave in nearly the same
// direction, so the lanes of a wave stay in step and their gathers of depth fall into a few cache lines.  Every sample is computed from
// its index (the contract).  The march is the plain one: a per-block nearest-z plane with an exact jump over blocks the ray passes in front
// of was built and measured slower at the default stride (profiles/ssr.txt), so `scratch` is not touched.
// kVec: normals, lit and out are 8-byte aligned with pitches that are multiples of 8 — a texel is one 8-byte access, otherwise two dwords.
#include <hip/hip_runtime.h>

#include "dither.hpp"
#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr int kSsW = 32, kSsH = 8;  // the trace kernel's tile: four waves of 8 x 8

namespace {
struct Ray {
    float s0x, s0y, k0, dsx, dsy, dk, L, jit, stride, wf, hf;
    SAH_DEV float t_of(float i) const { return ((i + jit) * stride) / L; }
    // the sample at parameter t: whether it lies inside the image, its texel and the ray's linear depth there
    SAH_DEV bool sample(float t, int& ix, int& iy, float& zr) const {
        const float sx = s0x + t * dsx, sy = s0y + t * dsy;
        const float k = k0 + t * dk;
        zr = 1.0f / k;
        const bool inside = (sx >= 0.0f) & (sx < wf) & (sy >= 0.0f) & (sy < hf);
        ix = inside ? (int)__builtin_floorf(sx) : 0, iy = inside ? (int)__builtin_floorf(sy) : 0;
        return inside;
    }
};

}  // namespace

template <bool kVec> __global__ void __launch_bounds__(256) k_ssr_trace(SsrArgs a) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const uint32_t tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;  // (rows folded into grid.x: no limit of 65,535 tile rows)
    const int x = (int)tile_x * kSsW + 8 * (tid >> 6) + (lane & 7), y = (int)(a.row_begin + tile_y * kSsH) + (lane >> 3);
    if (x >= (int)a.W || y >= (int)a.row_end) return;
    const bool only = (a.flags & SAH_SSR_REFLECTION_ONLY) != 0;
    const uint2 lit = load_texel8<kVec>(a.lit, x, y);
    uint2 res = only ? make_uint2(0u, 0u) : lit;  // what a pixel that passes through stores
    uint8_t* orow = const_cast<uint8_t*>(a.out.ptr) + (size_t)y * a.out.pitch + (size_t)x * 8;
    bool found = false;
    float t_hit = 0.0f, nv = 0.0f, rough = 0.0f;
    int hx = 0, hy = 0;
    float Rx = 0.0f, Ry = 0.0f, Rz = 0.0f;
    const float d = load_f32(a.depth, x, y);
    uint32_t dat = 0;
    if (d > 0.0f && a.intensity != 0.0f) {
        dat = *reinterpret_cast<const uint32_t*>(a.data.ptr + (size_t)y * a.data.pitch + (size_t)x * 4);
        rough = a.luts[256 + ((dat >> 8) & 0xffu)];
        const float z = a.z_near / d;
        const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
        const float Px = view_x(a, cx, z), Py = view_y(a, cy, z), Pz = -z;
        float Nx, Ny, Nz;
        view_normal(a, load_texel8<kVec>(a.normals, x, y), Nx, Ny, Nz);
        const bool finite = finite_f32(Px) && finite_f32(Py) && finite_f32(Pz) && finite_f32(Nx) && finite_f32(Ny) && finite_f32(Nz);
        if (finite && rough < a.max_roughness) {
            const float pl = __builtin_sqrtf((Px * Px + Py * Py) + Pz * Pz);
            const float Vx = Px / pl, Vy = Py / pl, Vz = Pz / pl;
            nv = (Nx * Vx + Ny * Vy) + Nz * Vz;
            const float nv2 = 2.0f * nv;
            Rx = Vx - nv2 * Nx, Ry = Vy - nv2 * Ny, Rz = Vz - nv2 * Nz;
            float len = a.max_distance;
            if (Rz > 0.0f) {
                const float lim = (z - a.z_near) / Rz;
                len = lim < len ? lim : len;
            }
            const float Ex = Px + Rx * len, Ey = Py + Ry * len, Ez = Pz + Rz * len;
            float ze = -Ez;
            ze = ze > a.z_near ? ze : a.z_near;
            Ray r;
            r.s0x = (((Px * a.p00) / z - a.p20) + 1.0f) * a.hw, r.s0y = (((Py * a.p11) / z - a.p21) + 1.0f) * a.hh;
            const float s1x = (((Ex * a.p00) / ze - a.p20) + 1.0f) * a.hw, s1y = (((Ey * a.p11) / ze - a.p21) + 1.0f) * a.hh;
            r.k0 = 1.0f / z;
            const float k1 = 1.0f / ze;
            r.dsx = s1x - r.s0x, r.dsy = s1y - r.s0y, r.dk = k1 - r.k0;
            const float ax = __builtin_fabsf(r.dsx), ay = __builtin_fabsf(r.dsy);
            r.L = ax > ay ? ax : ay;
            r.jit = (a.flags & SAH_SSR_JITTER) ? bayer4x4((uint32_t)x, (uint32_t)y) * 0.0625f : 0.0f;
            r.stride = a.stride, r.wf = (float)a.W, r.hf = (float)a.H;
            if ((ax < kScreenInf) & (ay < kScreenInf) & (r.L >= 1.0f) & (r.k0 < kScreenInf)) {
                const int steps = (int)a.max_steps;
                int hit_i = 0;
                for (int i = 1; i <= steps; i++) {
                    const float t = r.t_of((float)i);
                    if (t > 1.0f) break;
                    int ix, iy;
                    float zr;
                    if (!r.sample(t, ix, iy, zr)) break;
                    const float dt = load_f32(a.depth, ix, iy);
                    if (dt > 0.0f) {
                        const float dz = zr - a.z_near / dt;
                        if ((dz >= 0.0f) & (dz <= a.thickness)) {
                            hit_i = i;
                            break;
                        }
                    }
                }
                if (hit_i) {
                    float lo = r.t_of((float)(hit_i - 1)), hi = r.t_of((float)hit_i);
                    for (uint32_t s = 0; s < a.refine_steps; s++) {
                        const float mid = (lo + hi) * 0.5f;
                        int ix, iy;
                        float zr;
                        bool pass = r.sample(mid, ix, iy, zr);
                        const float dt = load_f32(a.depth, ix, iy);  // ((0, 0) outside the image: a texel of every image)
                        pass = pass && dt > 0.0f && zr >= a.z_near / dt;
                        hi = pass ? mid : hi, lo = pass ? lo : mid;
                    }
                    float zr;
                    r.sample(hi, hx, hy, zr);
                    t_hit = hi;
                    found = true;
                }
            }
        }
    }
    if (found) {
        const uint2 src = load_texel8<false>(a.source, hx, hy);
        const float sr = half_lo(src.x), sg = half_hi(src.x), sb = half_lo(src.y);
        float Hx, Hy, Hz;
        view_normal(a, load_texel8<false>(a.normals, hx, hy), Hx, Hy, Hz);
        const bool clean = all_nonneg_finite(sr, sg, sb);
        const bool facing = ((Hx * Rx + Hy * Ry) + Hz * Rz) < 0.0f;
        if (clean && facing) {
            const uint32_t col = *reinterpret_cast<const uint32_t*>(a.color.ptr + (size_t)y * a.color.pitch + (size_t)x * 4);
            const float metal = a.luts[256 + ((dat >> 16) & 0xffu)];
            const float m = 1.0f - clamp01(-nv);
            const float m2 = m * m;
            const float m5 = (m2 * m2) * m;
            const float rf = clamp01(1.0f - rough / a.max_roughness);
            const float u = ((float)hx + 0.5f) / (float)a.W, v = ((float)hy + 0.5f) / (float)a.H;
            const float e = sel_min(sel_min(u, 1.0f - u), sel_min(v, 1.0f - v));
            const float ef = clamp01(e / a.edge_fade);
            const float tf = clamp01(1.0f - t_hit);
            const float w = ((a.intensity * rf) * ef) * tf;
            const float s[3] = {sr, sg, sb};
            const float l[3] = {half_lo(lit.x), half_hi(lit.x), half_lo(lit.y)};
            uint32_t o[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float base = a.luts[(col >> (8 * c)) & 0xffu];
                const float f0 = 0.04f + (base - 0.04f) * metal;
                const float F = f0 + (1.0f - f0) * m5;
                const float g = w * F;
                const float term = g * s[c];
                o[c] = f2h(only ? term : l[c] + term);
            }
            const uint32_t alpha = only ? (uint32_t)f2h(w) : (lit.y >> 16);
            res = make_uint2(o[0] | (o[1] << 16), o[2] | (alpha << 16));
        }
    }
    store_texel8<kVec>(orow, res);
}

hipError_t launch_ssr(const SsrArgs& args, hipStream_t st) {
    if (args.row_end <= args.row_begin) return hipSuccess;
    SsrArgs a = args;
    const bool vec = planes_aligned({&a.normals, &a.lit, &a.out}, 8);
    // W, H < 2^31 and W * H < 2^32 (api_ssr.cpp): ceil(W / 32) * ceil(H / 8) stays below 2^29 however thin the frame, so grid.x holds every tile
    a.tiles_x = (a.W + kSsW - 1) / kSsW;
    const uint64_t tiles = (uint64_t)a.tiles_x * ((a.row_end - a.row_begin + kSsH - 1) / kSsH);
    if (tiles > 0x7fffffffull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(vec ? k_ssr_trace<true> : k_ssr_trace<false>, dim3((uint32_t)tiles), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
