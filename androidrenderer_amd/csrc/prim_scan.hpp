// Running triangle numbers, shared by the rasteriser's set-up (raster_setup.hip) and the ray tracer's build (rt.hip): the single-workgroup
// exclusive scan that turns per-primitive triangle counts into offsets, and the search from a running number back to its primitive.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "numerics.hpp"

namespace sah {

SAH_DEV uint32_t find_primitive(const uint32_t* tri_base, uint32_t n, uint32_t t) {  // last p with tri_base[p] <= t
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tri_base[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// out[i] = load(0) + .. + load(i - 1) for i < n, *total = the sum of all.  ONE workgroup of 1024 threads, every thread calls this; per
// round a thread takes kPer consecutive elements (the tile counts of four 4096^2 cascades are 16 K elements: at eight per thread 2
// rounds instead of 16, 18 -> 5 us).
template <uint32_t kPer, class Load>
SAH_DEV void block_exclusive_scan(uint32_t n, Load load, uint32_t* out, uint32_t* total) {
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024 * kPer) {
        const uint32_t i0 = base + tid * kPer;
        uint32_t v[kPer], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPer; k++) {
            const uint32_t i = i0 + k;
            v[k] = i < n ? load(i) : 0u;
            sum += v[k];
        }
        uint32_t incl = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if ((int)lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t wave_base = 0;
        for (uint32_t w = 0; w < wave; w++) wave_base += s_wave[w];
        const uint32_t carry = s_carry;
        uint32_t run = carry + wave_base + incl - sum;
#pragma unroll
        for (uint32_t k = 0; k < kPer; k++) {
            if (i0 + k < n) out[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (tid == 1023) s_carry = run;
        __syncthreads();
    }
    if (tid == 0) *total = s_carry;
}

}  // namespace sah
