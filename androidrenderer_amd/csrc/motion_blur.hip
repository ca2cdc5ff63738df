// Camera motion blur for gfx950 (include/sah_motion_blur.h): builder-owned arithmetic, restated by tests/motion_blur_ref.py.
//
// k_mb_tiles: one 256-thread workgroup per 16 x 16 tile of the render raster, one texel per thread.  A texel's key (l2, bit pattern) is one
// 64-bit unsigned number (l2 >= 0 is never a NaN, so its bits order as the floats do), plus one so that 0 can stand for a texel outside the
// image.  The greatest key crosses the wave by six xor-shuffles and the four waves through 32 bytes of LDS; the first thread stores the
// winner's raw pair.  A maximum of a total order: the result does not depend on how the reduction is shaped.
//
// k_mb_gather: a 256-thread workgroup covers 16 x 16 pixels of `out`, each of its four waves 16 x 4, one pixel per lane.  i(X) is monotone
// and sx <= 1, so the render texels of 16 adjacent pixels span at most 17 consecutive columns: at most two tiles per axis.  Sixteen threads
// read the 4 x 4 tile entries around the first pixel's tile (clamped to the grid) and turn them into keys, four threads reduce the four
// possible 3 x 3 neighbourhoods, and every pixel picks its own by its tile: the nine entries are read once per workgroup.
// Whether a pixel passes through is per pixel (the contract).  A wave whose every lane passes on the neighbour speed alone — the whole of
// a static-camera frame — only moves texels: on the wide path lanes 0..31 move two texels each as one 16-byte load and store.  Any other wave
// runs the tap loop, which gathers the vectors, the depth and the scene straight from memory through the caches.
// kVec: scene, depth, motion_vectors and out have pointers and pitches that are multiples of 16 — a texel of the scene is one 8-byte
// access and the copy branch moves 16 bytes; otherwise every access is a dword.
#include <hip/hip_runtime.h>

#include "dither.hpp"
#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr int kMbT = (int)SAH_MOTION_BLUR_TILE;
constexpr float kMbFar = 0x1p100f;

namespace {
// Velocity up to the clamp: the scaled vector of a pair of halfs and its squared length, zero where that is not finite
SAH_DEV float mb_scaled(const MotionBlurArgs& a, uint32_t m, float& ax, float& ay) {
    ax = (half_lo(m) + a.djx) * a.shutter;
    ay = (half_hi(m) + a.djy) * a.shutter;
    float l2 = ax * ax + ay * ay;
    if (!(l2 < kScreenInf)) ax = 0.0f, ay = 0.0f, l2 = 0.0f;
    return l2;
}
SAH_DEV uint64_t mb_key(const MotionBlurArgs& a, uint32_t m) {
    float ax, ay;
    const float l2 = mb_scaled(a, m, ax, ay);
    return ((uint64_t)__builtin_bit_cast(uint32_t, l2) << 32) | m;
}
struct MbVelocity {
    float x, y, speed;
};
SAH_DEV MbVelocity mb_velocity(const MotionBlurArgs& a, uint32_t m) {
    float ax, ay;
    const float l = __builtin_sqrtf(mb_scaled(a, m, ax, ay));
    if (l > a.max_blur) {
        const float s = a.max_blur / l;
        return {ax * s, ay * s, a.max_blur};
    }
    return {ax, ay, l};
}
// Surface: the linear depth of a texel, a large finite one without a surface
SAH_DEV float mb_linear_depth(const MotionBlurArgs& a, float d) {
    const float z = d > 0.0f ? a.z_near / d : kMbFar;
    return z < kMbFar ? z : kMbFar;
}
SAH_DEV float mb_cone(float d, float s) { return clamp01(1.0f - d / s); }
SAH_DEV float mb_cyl(float d, float s) {
    const float e0 = 0.95f * s, e1 = 1.05f * s;
    const float y = clamp01((e1 - d) / (e1 - e0));
    return (y * y) * (3.0f - 2.0f * y);
}
}  // namespace

__global__ void __launch_bounds__(256) k_mb_tiles(MotionBlurArgs a) {
    __shared__ uint64_t s_key[4];
    const int tid = (int)threadIdx.x;
    const uint32_t row = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - row * a.tiles_x, tile_y = a.tile_row_begin + row;
    const int x = (int)tile_x * kMbT + (tid & 15), y = (int)tile_y * kMbT + (tid >> 4);
    uint64_t key = 0;  // a texel outside the image takes no part
    if (x < (int)a.w && y < (int)a.h) key = mb_key(a, load_u32(a.mv, x, y)) + 1;
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const uint64_t other = __shfl_xor(key, off);
        key = other > key ? other : key;
    }
    if ((tid & 63) == 0) s_key[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 4; i++) key = s_key[i] > key ? s_key[i] : key;
        // (the tile's first texel is inside the image, so key >= 1)
        *reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(a.tiles.ptr) + (size_t)tile_y * a.tiles.pitch + (size_t)tile_x * 4) = (uint32_t)(key - 1);
    }
}

template <bool kVec> __global__ void __launch_bounds__(256) k_mb_gather(MotionBlurArgs a) {
    __shared__ uint64_t s_key[16];
    __shared__ uint32_t s_neighbour[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = (int)a.w, h = (int)a.h, W = (int)a.W, row_end = (int)a.row_end;
    const uint32_t group_y = blockIdx.x / a.groups_x, group_x = blockIdx.x - group_y * a.groups_x;  // (rows folded into grid.x, as k_ssr_trace)
    const int X0 = (int)group_x * kMbT, Y0 = (int)(a.row_begin + group_y * kMbT);
    // the tile of the workgroup's first pixel; every pixel's tile is that one or the next, per axis
    const int bx0 = clampi(floor_i32(sample_position(X0, a.sx, a.jx)), w) >> 4;
    const int by0 = clampi(floor_i32(sample_position(Y0, a.sy, a.jy)), h) >> 4;
    if (tid < 16) {
        const int tx = clampi(bx0 - 1 + (tid & 3), (int)a.tiles_x), ty = clampi(by0 - 1 + (tid >> 2), (int)a.tiles_y);
        s_key[tid] = mb_key(a, load_u32(a.tiles, tx, ty));
    }
    __syncthreads();
    if (tid < 4) {
        const int ox = tid & 1, oy = tid >> 1;
        uint64_t best = 0;
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
                const uint64_t k = s_key[(oy + dy) * 4 + ox + dx];
                best = k > best ? k : best;
            }
        s_neighbour[tid] = (uint32_t)best;
    }
    __syncthreads();
    const int X = X0 + (tid & 15), Y = Y0 + (tid >> 4);
    const bool inside = X < W && Y < row_end;
    const float ux = sample_position(min(X, W - 1), a.sx, a.jx), uy = sample_position(min(Y, row_end - 1), a.sy, a.jy);
    const int i = clampi(floor_i32(ux), w), j = clampi(floor_i32(uy), h);
    const MbVelocity vn = mb_velocity(a, s_neighbour[min((i >> 4) - bx0, 1) + 2 * min((j >> 4) - by0, 1)]);
    const bool moving = inside && !(vn.speed < a.min_velocity);
    if (!wave_any(moving)) {  // nothing but a copy: the static-camera frame
        if (kVec) {
            const int cx = X0 + 2 * (lane & 7), cy = Y0 + 4 * wave + (lane >> 3);
            if (lane < 32 && cx < W && cy < row_end) {
                const uint8_t* src = a.scene.ptr + (size_t)cy * a.scene.pitch + (size_t)cx * 8;
                uint8_t* dst = const_cast<uint8_t*>(a.out.ptr) + (size_t)cy * a.out.pitch + (size_t)cx * 8;
                if (cx + 1 < W) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
                else *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(src);
            }
        } else if (inside) {
            store_texel8<false>(a.out, X, Y, load_texel8<false>(a.scene, X, Y));
        }
        return;
    }
    if (!inside) return;
    const uint2 own = load_texel8<kVec>(a.scene, X, Y);
    uint2 res = own;
    // (spelled out, not half_lo / half_hi: through the helpers this one line leaves the kernel another register assignment)
    const float c[3] = {h2f((uint16_t)(own.x & 0xffffu)), h2f((uint16_t)(own.x >> 16)), h2f((uint16_t)(own.y & 0xffffu))};
    if (moving && all_nonneg_finite(c[0], c[1], c[2])) {
        const MbVelocity vp = mb_velocity(a, load_u32(a.mv, i, j));
        const float zp = mb_linear_depth(a, load_f32(a.depth, i, j));
        const float dith = (a.flags & SAH_MOTION_BLUR_DITHER) ? (bayer4x4((uint32_t)X, (uint32_t)Y) - 7.5f) * 0.0625f : 0.0f;
        const float wf = (float)a.w, hf = (float)a.h, Wf = (float)a.W, Hf = (float)a.H;
        float sw = 0.0f, acc[3] = {0.0f, 0.0f, 0.0f};
        const int taps = (int)a.sample_count;
        for (int k = 0; k < taps; k++) {
            const float t = (((float)k + 0.5f) + dith) / a.nf - 0.5f;
            const float ex = vn.x * t, ey = vn.y * t;
            const float px = ux + ex, py = uy + ey;
            if (!((px >= 0.0f) & (px < wf) & (py >= 0.0f) & (py < hf))) continue;
            const float qx = px * a.rx, qy = py * a.ry;
            if (!((qx >= 0.0f) & (qx < Wf) & (qy >= 0.0f) & (qy < Hf))) continue;
            // (the min: float(w) rounds up for some w > 2^24, and no address may follow it)
            const int ti = min((int)__builtin_floorf(px), w - 1), tj = min((int)__builtin_floorf(py), h - 1);
            const int si = min((int)__builtin_floorf(qx), W - 1), sj = min((int)__builtin_floorf(qy), (int)a.H - 1);
            const uint2 st = load_texel8<kVec>(a.scene, si, sj);
            const float s[3] = {half_lo(st.x), half_hi(st.x), half_lo(st.y)};
            if (!all_nonneg_finite(s[0], s[1], s[2])) continue;
            const MbVelocity vs = mb_velocity(a, load_u32(a.mv, ti, tj));
            const float zs = mb_linear_depth(a, load_f32(a.depth, ti, tj));
            const float d = __builtin_sqrtf(ex * ex + ey * ey);
            const float f = clamp01(1.0f - (zs - zp) / a.depth_extent), g = clamp01(1.0f - (zp - zs) / a.depth_extent);
            const float wk = (f * mb_cone(d, vs.speed) + g * mb_cone(d, vp.speed)) + (2.0f * mb_cyl(d, vs.speed)) * mb_cyl(d, vp.speed);
            if (wk != 0.0f) {
                sw = sw + wk;
#pragma unroll
                for (int ch = 0; ch < 3; ch++) acc[ch] = acc[ch] + wk * (s[ch] - c[ch]);
            }
        }
        if (sw != 0.0f) {
            float r[3], o[3];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) r[ch] = acc[ch] / sw, o[ch] = c[ch] + r[ch];
            if (all_finite(o[0], o[1], o[2])) {
                const uint32_t h0 = r[0] != 0.0f ? (uint32_t)f2h(o[0]) : own.x & 0xffffu;
                const uint32_t h1 = r[1] != 0.0f ? (uint32_t)f2h(o[1]) : own.x >> 16;
                const uint32_t h2 = r[2] != 0.0f ? (uint32_t)f2h(o[2]) : own.y & 0xffffu;
                res = make_uint2(h0 | (h1 << 16), h2 | (own.y & 0xffff0000u));
            }
        }
    }
    store_texel8<kVec>(a.out, X, Y, res);
}

hipError_t launch_motion_blur(const MotionBlurArgs& args, hipStream_t st) {
    if (args.row_end <= args.row_begin) return hipSuccess;
    MotionBlurArgs a = args;
    const bool vec = planes_aligned({&a.scene, &a.depth, &a.mv, &a.out}, 16);
    // w, h, W, H < 2^31 and w * h, W * H < 2^32 (api_motion_blur.cpp): both tile counts stay below 2^31 however thin the frame
    a.groups_x = (a.W + kMbT - 1) / kMbT;
    const uint64_t groups = (uint64_t)a.groups_x * ((a.row_end - a.row_begin + kMbT - 1) / kMbT);
    const uint64_t tiles = (uint64_t)a.tiles_x * (a.tile_row_end - a.tile_row_begin);
    if (groups > 0x7fffffffull || tiles > 0x7fffffffull || !tiles) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_mb_tiles, dim3((uint32_t)tiles), dim3(256), 0, st, a);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(vec ? k_mb_gather<true> : k_mb_gather<false>, dim3((uint32_t)groups), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
