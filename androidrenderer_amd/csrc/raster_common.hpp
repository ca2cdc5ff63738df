// Device code shared by the two stages of the scene rasteriser (raster_setup.hip, raster_tiles.hip): the record helpers, the exact edge
// arithmetic in both of its forms (whole tiles for binning, pixels and 8x8 blocks for the tile kernel) and the wave-level helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "numerics.hpp"
#include "raster_args.hpp"

namespace sah {

constexpr int kTile = (int)kRasterTile;  // pixels per tile edge

// ---- records --------------------------------------------------------------------------------------------------------------------------
SAH_DEV void mark_empty(RasterRecord& r) { r.x0 = 1; r.x1 = 0; r.y0 = 1; r.y1 = 0; }
SAH_DEV bool is_empty(const RasterRecord& r) { return r.x0 > r.x1; }
SAH_DEV uint32_t record_count(const RasterArgs& a) {  // direct slots + appended fans, clamped to the buffer
    const uint64_t n = (uint64_t)a.counters[C_TRIS] * a.num_views + a.counters[C_RECORDS];
    return n < a.record_capacity ? (uint32_t)n : a.record_capacity;
}

// ---- wave helpers ---------------------------------------------------------------------------------------------------------------------
// One atomic per wave instead of one per lane (the counters are single addresses: per-lane atomics serialise in L2).
SAH_DEV uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// Adds the workgroup's sum of `local[i]` to counter[i], one global atomic per counter and workgroup (every thread must call this;
// `s_acc` is N words of LDS).  The counters are single addresses and such atomics complete at a few tens of nanoseconds each, device
// wide: per-wave flushes of four counters cost more than the set-up work itself.
template <int N>
SAH_DEV void block_flush(uint32_t* counter, const uint32_t (&local)[N], uint32_t* s_acc) {
    if (threadIdx.x < N) s_acc[threadIdx.x] = 0;
    __syncthreads();
    for (int i = 0; i < N; i++) {
        const uint32_t total = wave_sum(local[i]);
        if ((threadIdx.x & 63u) == 0 && total) atomicAdd(&s_acc[i], total);
    }
    __syncthreads();
    if (threadIdx.x < N && s_acc[threadIdx.x]) atomicAdd(&counter[threadIdx.x], s_acc[threadIdx.x]);
}
// slot for the lanes that `want` one: the first of them adds the count, the rest take consecutive slots
SAH_DEV uint32_t wave_alloc(uint32_t* counter, bool want) {
    const uint64_t mask = __ballot(want);
    uint32_t slot = 0;
    if (want) {
        const uint32_t lane = threadIdx.x & 63u;
        const int leader = __builtin_ctzll(mask);
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__builtin_popcountll(mask));
        base = __shfl(base, leader, 64);
        slot = base + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
    }
    return slot;
}
SAH_DEV uint32_t readlane(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
SAH_DEV float readlane(float v, int src) { return __uint_as_float(readlane(__float_as_uint(v), src)); }
SAH_DEV double readlane(double v, int src) {
    const uint64_t bits = __builtin_bit_cast(uint64_t, v);
    return __builtin_bit_cast(double, (uint64_t)readlane((uint32_t)bits, src) | ((uint64_t)readlane((uint32_t)(bits >> 32), src) << 32));
}

// ---- edge functions -------------------------------------------------------------------------------------------------------------------
// Edge functions in fp64.  Window coordinates are integers below 2^24.1 (guard band 16 half-viewports of at most 8192 pixels, 8
// sub-pixel bits), so every product and sum below is an integer of magnitude < 2^52: fp64 evaluates it EXACTLY, and (float)E is the
// single correctly rounded conversion of the integer the specification talks about.  E_i(px, py) = c_i + px a_i + py b_i.
struct EdgeSetup {
    double a[3], b[3], c[3];
    uint32_t tl;        // bit i: edge i is a top or left edge
    double zc, zx, zy;  // depth plane z(px, py) = zc + px zx + py zy
    float inv_area;
    uint32_t seq, cutout;
};
// lane `src`'s set-up, in scalar registers of every lane of the wave
SAH_DEV EdgeSetup broadcast(const EdgeSetup& e, int src) {
    EdgeSetup r;
    for (int i = 0; i < 3; i++) { r.a[i] = readlane(e.a[i], src); r.b[i] = readlane(e.b[i], src); r.c[i] = readlane(e.c[i], src); }
    r.zc = readlane(e.zc, src); r.zx = readlane(e.zx, src); r.zy = readlane(e.zy, src);
    r.tl = readlane(e.tl, src);
    r.inv_area = readlane(e.inv_area, src);
    r.seq = readlane(e.seq, src);
    r.cutout = readlane(e.cutout, src);
    return r;
}
SAH_DEV EdgeSetup edge_setup(const RasterRecord& rec) {
    EdgeSetup e;
    e.tl = 0;
    e.seq = rec.seq;
    e.cutout = rec.cutout;
    for (int i = 0; i < 3; i++) {
        const int va = (i + 1) % 3, vb = (i + 2) % 3;  // edge i runs from vertex i+1 to vertex i+2
        const int32_t dx = rec.X[vb] - rec.X[va], dy = rec.Y[vb] - rec.Y[va];
        e.tl |= ((dy < 0) | ((dy == 0) & (dx > 0))) ? 1u << i : 0u;
        e.a[i] = -256.0 * (double)dy;
        e.b[i] = 256.0 * (double)dx;
        e.c[i] = (double)dx * (double)(128 - rec.Y[va]) - (double)dy * (double)(128 - rec.X[va]);
    }
    const double area = (double)(rec.X[1] - rec.X[0]) * (double)(rec.Y[2] - rec.Y[0]) - (double)(rec.X[2] - rec.X[0]) * (double)(rec.Y[1] - rec.Y[0]);
    e.inv_area = 1.0f / (float)area;
    // depth plane: sum_i E_i(px, py) z_i / area, coefficient by coefficient in fp64 (every operator rounded)
    const double inv = 1.0 / area, z0 = (double)rec.z[0], z1 = (double)rec.z[1], z2 = (double)rec.z[2];
    e.zc = ((e.c[0] * z0 + e.c[1] * z1) + e.c[2] * z2) * inv;
    e.zx = ((e.a[0] * z0 + e.a[1] * z1) + e.a[2] * z2) * inv;
    e.zy = ((e.b[0] * z0 + e.b[1] * z1) + e.b[2] * z2) * inv;
    return e;
}
// coverage of pixel (px, py); v = the three edge functions
SAH_DEV bool cover(const EdgeSetup& e, int32_t px, int32_t py, double v[3]) {
    const double x = (double)px, y = (double)py;
    bool inside = true;
    for (int i = 0; i < 3; i++) {
        v[i] = __builtin_fma(x, e.a[i], __builtin_fma(y, e.b[i], e.c[i]));
        // (bitwise, here and in the block sweep: the short-circuit forms compiled to three nested exec-mask regions per pixel in the
        //  innermost loops)
        inside = inside & ((v[i] > 0.0) | ((v[i] == 0.0) & (((e.tl >> i) & 1u) != 0u)));
    }
    return inside;
}
// screen-space barycentrics from the edge functions
SAH_DEV void barycentrics(const EdgeSetup& e, const double v[3], float b[3]) {
    for (int i = 0; i < 3; i++) b[i] = (float)v[i] * e.inv_area;
}
SAH_DEV float fragment_depth(const EdgeSetup& e, int32_t px, int32_t py) {
    const float z = (float)__builtin_fma((double)py, e.zy, __builtin_fma((double)px, e.zx, e.zc));
    return __builtin_fminf(__builtin_fmaxf(z, 0.0f), 1.0f);  // depth clamp (shadow PSO) / [0,1] viewport range; NaN -> 0
}

// No pixel centre of the 64x64 tile at pixel (x0, y0) is inside the record's triangle: some edge function is negative even at the
// tile corner that favours it.  Exact (fp64 on integers below 2^52, see EdgeSetup above).
SAH_DEV bool tile_outside(const RasterRecord& rec, int32_t x0, int32_t y0) {
    for (int i = 0; i < 3; i++) {
        const int va = (i + 1) % 3, vb = (i + 2) % 3;
        const int32_t dx = rec.X[vb] - rec.X[va], dy = rec.Y[vb] - rec.Y[va];
        // E(px, py) = dx ((256 py + 128) - Ya) - dy ((256 px + 128) - Xa): largest where py is at the dx > 0 end and px at the dy < 0 end
        const int32_t py = dx > 0 ? y0 + kTile - 1 : y0, px = dy < 0 ? x0 + kTile - 1 : x0;
        const double e = (double)dx * (double)(256 * py + 128 - rec.Y[va]) - (double)dy * (double)(256 * px + 128 - rec.X[va]);
        if (e < 0.0) return true;
    }
    return false;
}

}  // namespace sah
