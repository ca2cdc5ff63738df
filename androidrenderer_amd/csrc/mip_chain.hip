// The mip-chain generator for gfx950 (include/sah_mip_chain.h): AMD's single-pass downsampler as the reference's four shaders instantiate it,
//   RenderCore/shaders/util/mip_chain_generator_{D32F_min,R16F,RGBA16F,B10G11R11F}.comp over RenderCore/extern/spd/ffx_spd.h:855-1283
//   (host: RenderCore/render/mip_chain_generator.cpp:60-177).
//
// One launch writes every level.  A 256-thread workgroup owns a 64 x 64 source tile: each thread samples four level-0 texels, and the
// 2 x 2 reductions of levels 1-5 are exchanges inside the quads of lanes 4k .. 4k+3 (DPP quad permutes, no LDS traffic for the exchange
// itself) under SPD's lane-to-texel map ARmpRed8x8 — lane bits 0 and 1 are the low bits of x and y, so lane ^ 1 is the right neighbour,
// lane ^ 2 the one below and lane ^ 3 the diagonal.  Between levels the survivors (a quarter each time) go through a 16 x 16 LDS array
// in the shader's own skewed layout.  Each workgroup then signs a device-wide counter; the one that draws the last ticket reads the
// stored level 5 back and runs the same stages again for levels 6-11.
//
// Cross-workgroup hand-over: every thread releases its stores at agent scope (its own wave's stores have reached L2) before the
// workgroup barrier in front of the ticket, thread 0 takes the ticket with an acquire-release add, and every thread of the electing
// workgroup acquires at agent scope behind the second barrier before its first load of level 5.  All global writes are per-lane stores.
//
// The channel count is a template parameter: the depth and R16 chains carry one half per texel, B10G11R11 three, RGBA16F four.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "numerics.hpp"
#include "r11g11b10.hpp"

namespace sah {

namespace {

template <int kKind> struct MipFormat;
template <> struct MipFormat<kMipChainR32Min> {  // imgSrc: D32 / R32 sampled as fp32; imgDst: r32f
    static constexpr int C = 1, kTexel = 4;
    static constexpr bool kMin = true;
    static SAH_DEV void load(const uint8_t* p, float (&t)[C]) { t[0] = *reinterpret_cast<const float*>(p); }
    static SAH_DEV void load_half(const uint8_t* p, _Float16 (&t)[C]) { t[0] = __builtin_bit_cast(_Float16, f2h(*reinterpret_cast<const float*>(p))); }
    static SAH_DEV void store(uint8_t* p, const _Float16 (&t)[C]) { *reinterpret_cast<float*>(p) = (float)t[0]; }
};
template <> struct MipFormat<kMipChainR16> {
    static constexpr int C = 1, kTexel = 2;
    static constexpr bool kMin = false;
    static SAH_DEV void load_half(const uint8_t* p, _Float16 (&t)[C]) { t[0] = *reinterpret_cast<const _Float16*>(p); }
    static SAH_DEV void load(const uint8_t* p, float (&t)[C]) { t[0] = (float)*reinterpret_cast<const _Float16*>(p); }
    static SAH_DEV void store(uint8_t* p, const _Float16 (&t)[C]) { *reinterpret_cast<_Float16*>(p) = t[0]; }
};
template <> struct MipFormat<kMipChainRGBA16> {
    static constexpr int C = 4, kTexel = 8;
    static constexpr bool kMin = false;
    static SAH_DEV void load_half(const uint8_t* p, _Float16 (&t)[C]) {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
        t[0] = __builtin_bit_cast(_Float16, (uint16_t)(w.x & 0xffffu)), t[1] = __builtin_bit_cast(_Float16, (uint16_t)(w.x >> 16));
        t[2] = __builtin_bit_cast(_Float16, (uint16_t)(w.y & 0xffffu)), t[3] = __builtin_bit_cast(_Float16, (uint16_t)(w.y >> 16));
    }
    static SAH_DEV void load(const uint8_t* p, float (&t)[C]) {
        _Float16 h[C];
        load_half(p, h);
        for (int c = 0; c < C; c++) t[c] = (float)h[c];
    }
    static SAH_DEV void store(uint8_t* p, const _Float16 (&t)[C]) {
        uint2 w;
        w.x = (uint32_t)__builtin_bit_cast(uint16_t, t[0]) | ((uint32_t)__builtin_bit_cast(uint16_t, t[1]) << 16);
        w.y = (uint32_t)__builtin_bit_cast(uint16_t, t[2]) | ((uint32_t)__builtin_bit_cast(uint16_t, t[3]) << 16);
        *reinterpret_cast<uint2*>(p) = w;
    }
};
template <> struct MipFormat<kMipChainR11G11B10> {  // (the shader's fourth channel is the constant alpha of the load and is dropped by the store)
    static constexpr int C = 3, kTexel = 4;
    static constexpr bool kMin = false;
    static SAH_DEV void load_half(const uint8_t* p, _Float16 (&t)[C]) {
        Hn c[3];
        decode_r11g11b10(*reinterpret_cast<const uint32_t*>(p), c);
        for (int k = 0; k < C; k++) t[k] = c[k].v;
    }
    static SAH_DEV void load(const uint8_t* p, float (&t)[C]) {
        _Float16 h[C];
        load_half(p, h);
        for (int c = 0; c < C; c++) t[c] = (float)h[c];
    }
    static SAH_DEV void store(uint8_t* p, const _Float16 (&t)[C]) {
        *reinterpret_cast<uint32_t*>(p) = encode_r11g11b10(Hn::raw(t[0]), Hn::raw(t[1]), Hn::raw(t[2]));
    }
};

// SpdReduce4H of the four shaders: min(min(v0, v1), min(v2, v3)) (minNum: a NaN operand yields the other) or (((v0 + v1) + v2) + v3) * 0.25
template <bool kMin> SAH_DEV _Float16 reduce4(_Float16 v0, _Float16 v1, _Float16 v2, _Float16 v3) {
    if (kMin) return __builtin_fminf16(__builtin_fminf16(v0, v1), __builtin_fminf16(v2, v3));
    return (((v0 + v1) + v2) + v3) * (_Float16)0.25f;
}

// the value of lane ^ 1, ^ 2, ^ 3: quad_perm [1,0,3,2], [2,3,0,1], [3,2,1,0].  Every caller runs with whole quads active.
template <int kCtrl> SAH_DEV _Float16 quad_swap(_Float16 v) {
    const int u = (int)__builtin_bit_cast(uint16_t, v);
    return __builtin_bit_cast(_Float16, (uint16_t)__builtin_amdgcn_mov_dpp(u, kCtrl, 0xf, 0xf, true));
}
// SpdReduceQuadH (:861-868): own, horizontal, vertical, diagonal.  The result is used by the lanes 4k alone, for which these are own, right,
// below, diagonal.
template <class F> SAH_DEV void reduce_quad(_Float16 (&v)[F::C]) {
#pragma unroll
    for (int c = 0; c < F::C; c++) v[c] = reduce4<F::kMin>(v[c], quad_swap<0xB1>(v[c]), quad_swap<0x4E>(v[c]), quad_swap<0x1B>(v[c]));
}

SAH_DEV uint32_t wrap_repeat(int i, uint32_t n) {
    const int m = i % (int)n;
    return (uint32_t)(m < 0 ? m + (int)n : m);
}

// SpdLoadSourceImageH: textureLod(imgSrc, p * invInputSize + invInputSize, 0) under the LINEAR / REPEAT sampler, then AH4()
template <class F> SAH_DEV void sample_source(const MipChainArgs& a, uint32_t tx, uint32_t ty, _Float16 (&out)[F::C]) {
    const float u = (float)tx * a.inv_w + a.inv_w, v = (float)ty * a.inv_h + a.inv_h;
    const float px = u * (float)a.src_w - 0.5f, py = v * (float)a.src_h - 0.5f;  // (finite: tx, ty < 2^13)
    const float fx0 = __builtin_floorf(px), fy0 = __builtin_floorf(py);
    const float fx = px - fx0, fy = py - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    const uint32_t xa = wrap_repeat(x0, a.src_w), xb = wrap_repeat(x0 + 1, a.src_w);
    const uint32_t ya = wrap_repeat(y0, a.src_h), yb = wrap_repeat(y0 + 1, a.src_h);
    const uint8_t* ra = a.src.ptr + (size_t)ya * a.src.pitch;
    const uint8_t* rb = a.src.ptr + (size_t)yb * a.src.pitch;
    float t00[F::C], t10[F::C], t01[F::C], t11[F::C];
    F::load(ra + (size_t)xa * F::kTexel, t00);
    F::load(ra + (size_t)xb * F::kTexel, t10);
    F::load(rb + (size_t)xa * F::kTexel, t01);
    F::load(rb + (size_t)xb * F::kTexel, t11);
    const float wx0 = 1.0f - fx, wy0 = 1.0f - fy;
    const float w00 = wx0 * wy0, w10 = fx * wy0, w01 = wx0 * fy, w11 = fx * fy;
#pragma unroll
    for (int c = 0; c < F::C; c++) {
        float acc = __builtin_fmaf(w00, t00[c], 0.0f);
        acc = __builtin_fmaf(w10, t10[c], acc);
        acc = __builtin_fmaf(w01, t01[c], acc);
        acc = __builtin_fmaf(w11, t11[c], acc);
        out[c] = __builtin_bit_cast(_Float16, f2h(acc));
    }
}

// SpdStoreH: imageStore(imgDst[mip], p, value) — dropped outside the slot's extent
template <class F> SAH_DEV void store_level(const MipChainArgs& a, uint32_t mip, uint32_t px, uint32_t py, const _Float16 (&v)[F::C]) {
    if (px >= a.slot_w[mip] || py >= a.slot_h[mip]) return;
    F::store(const_cast<uint8_t*>(a.slot[mip].ptr) + (size_t)py * a.slot[mip].pitch + (size_t)px * F::kTexel, v);
}
// SpdLoadH: imageLoad(imgDst[5], p) — 0 outside the extent
template <class F> SAH_DEV void load_level5(const MipChainArgs& a, uint32_t px, uint32_t py, _Float16 (&v)[F::C]) {
#pragma unroll
    for (int c = 0; c < F::C; c++) v[c] = (_Float16)0.0f;
    if (px >= a.slot_w[5] || py >= a.slot_h[5]) return;
    F::load_half(a.slot[5].ptr + (size_t)py * a.slot[5].pitch + (size_t)px * F::kTexel, v);
}

template <class F> struct Mid {  // spdIntermediate[16][16], indexed [x][y] as the shader does
    _Float16 v[16][16][F::C];
    SAH_DEV void put(uint32_t x, uint32_t y, const _Float16 (&t)[F::C]) {
#pragma unroll
        for (int c = 0; c < F::C; c++) v[x][y][c] = t[c];
    }
    SAH_DEV void get(uint32_t x, uint32_t y, _Float16 (&t)[F::C]) const {
#pragma unroll
        for (int c = 0; c < F::C; c++) t[c] = v[x][y][c];
    }
};

// SpdDownsampleNextFourH (:1239-1256): four more levels from the 16 x 16 values in LDS, first level `base`, for the workgroup at (wx, wy)
template <class F> SAH_DEV void next_four(const MipChainArgs& a, Mid<F>& mid, uint32_t x, uint32_t y, uint32_t wx, uint32_t wy, uint32_t tid, uint32_t base) {
    _Float16 v[F::C];
    if (a.mips <= base) return;
    __syncthreads();
    mid.get(x, y, v);  // SpdDownsampleMip_2H :1090-1097
    reduce_quad<F>(v);
    if ((tid & 3u) == 0) {
        store_level<F>(a, base, wx * 8 + x / 2, wy * 8 + y / 2, v);
        mid.put(x + (y / 2) % 2, y, v);
    }
    if (a.mips <= base + 1) return;
    __syncthreads();
    if (tid < 64) {  // SpdDownsampleMip_3H :1131-1141
        mid.get(x * 2 + y % 2, y * 2, v);
        reduce_quad<F>(v);
        if ((tid & 3u) == 0) {
            store_level<F>(a, base + 1, wx * 4 + x / 2, wy * 4 + y / 2, v);
            mid.put(x * 2 + y / 2, y * 2, v);
        }
    }
    if (a.mips <= base + 2) return;
    __syncthreads();
    if (tid < 16) {  // SpdDownsampleMip_4H :1166-1176
        mid.get(x * 4 + y, y * 4, v);
        reduce_quad<F>(v);
        if ((tid & 3u) == 0) {
            store_level<F>(a, base + 2, wx * 2 + x / 2, wy * 2 + y / 2, v);
            mid.put(x / 2 + y, 0, v);
        }
    }
    if (a.mips <= base + 3) return;
    __syncthreads();
    if (tid < 4) {  // SpdDownsampleMip_5H :1196-1205
        mid.get(tid, 0, v);
        reduce_quad<F>(v);
        if (tid == 0) store_level<F>(a, base + 3, wx, wy, v);
    }
}

template <int kKind> __global__ void __launch_bounds__(256) k_mip_chain(MipChainArgs a) {
    using F = MipFormat<kKind>;
    constexpr int C = F::C;
    __shared__ Mid<F> mid;
    __shared__ uint32_t s_ticket;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wx = blockIdx.x, wy = blockIdx.y;
    // ARmpRed8x8 (ffx_a.h): x = a0 + 2 a3 + 4 a4, y = a1 + 2 a2 + 4 a5 of the lane index a; waves 1-3 take the other 8 x 8 blocks (:1265-1267)
    const uint32_t x = ((lane & 1u) | ((lane >> 2) & 6u)) + 8u * ((tid >> 6) & 1u);
    const uint32_t y = (((lane >> 1) & 3u) | ((lane >> 3) & 4u)) + 8u * (tid >> 7);

    // SpdDownsampleMips_0_1_IntrinsicsH (:956-1002)
    _Float16 v[4][C];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t ox = 16u * (q & 1), oy = 16u * (q >> 1);
        sample_source<F>(a, wx * 64 + 2 * (x + ox), wy * 64 + 2 * (y + oy), v[q]);
        store_level<F>(a, 0, wx * 32 + x + ox, wy * 32 + y + oy, v[q]);
    }
    if (a.mips <= 1) return;
#pragma unroll
    for (int q = 0; q < 4; q++) reduce_quad<F>(v[q]);
    if ((tid & 3u) == 0) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t ox = 8u * (q & 1), oy = 8u * (q >> 1);
            store_level<F>(a, 1, wx * 16 + x / 2 + ox, wy * 16 + y / 2 + oy, v[q]);
            mid.put(x / 2 + ox, y / 2 + oy, v[q]);
        }
    }
    next_four<F>(a, mid, x, y, wx, wy, tid, 2);
    if (a.mips < 7) return;

    // SpdExitWorkgroup (:1273-1277): the last workgroup to sign the counter goes on
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != a.num_workgroups - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (tid == 0) __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // SpdResetAtomicCounter

    // SpdDownsampleMips_6_7H (:1209-1237): level 6 from STORED level 5 — (0,0) (0,1) (1,0) (1,1): below before right
    _Float16 w[4][C];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t tx = x * 4 + 2u * (q & 1), ty = y * 4 + 2u * (q >> 1);
        _Float16 t0[C], t1[C], t2[C], t3[C];
        load_level5<F>(a, tx, ty, t0);
        load_level5<F>(a, tx, ty + 1, t1);
        load_level5<F>(a, tx + 1, ty, t2);
        load_level5<F>(a, tx + 1, ty + 1, t3);
#pragma unroll
        for (int c = 0; c < C; c++) w[q][c] = reduce4<F::kMin>(t0[c], t1[c], t2[c], t3[c]);
        store_level<F>(a, 6, x * 2 + (q & 1), y * 2 + (q >> 1), w[q]);
    }
    if (a.mips < 8) return;
    // (the shader needs no barrier here; this one orders a stray store of level 6 before a stray store of level 7 to the same texel of
    // level 1 when both levels are missing — different threads write them)
    __syncthreads();
    _Float16 r[C];
#pragma unroll
    for (int c = 0; c < C; c++) r[c] = reduce4<F::kMin>(w[0][c], w[1][c], w[2][c], w[3][c]);
    store_level<F>(a, 7, x, y, r);
    mid.put(x, y, r);
    next_four<F>(a, mid, x, y, 0, 0, tid, 8);
}

}  // namespace

hipError_t launch_mip_chain(const MipChainArgs& a, MipChainKind kind, hipStream_t st) {
    const dim3 grid((a.src_w + 63) / 64, (a.src_h + 63) / 64), block(256);
    switch (kind) {
        case kMipChainR32Min: hipLaunchKernelGGL(k_mip_chain<kMipChainR32Min>, grid, block, 0, st, a); break;
        case kMipChainR16: hipLaunchKernelGGL(k_mip_chain<kMipChainR16>, grid, block, 0, st, a); break;
        case kMipChainRGBA16: hipLaunchKernelGGL(k_mip_chain<kMipChainRGBA16>, grid, block, 0, st, a); break;
        case kMipChainR11G11B10: hipLaunchKernelGGL(k_mip_chain<kMipChainR11G11B10>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

}  // namespace sah
