// The resolve of the VRSAA frame (include/sah_vrs.h): 2W x 2H RGBA16F down to W x H, the mean of each 2 x 2 block.  A streaming kernel: a
// thread makes four output pixels from two 64-byte row segments (16-byte loads) and stores 32 bytes; planes that do not allow 16-byte
// accesses take one pixel per thread with 8-byte accesses.
#include <hip/hip_runtime.h>

#include "../../include/sah_vrs.h"
#include "launch.hpp"
#include "params.hpp"

namespace sah {
namespace {

// one half of each of the block's four texels (a, b the upper pair, left first): ((a + b) + (c + d)) * 0.25f, stored as a half, NaN as 0x7e00
__device__ __forceinline__ uint32_t resolve_half(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    auto f = [](uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); };
    const float r = ((f(a) + f(b)) + (f(c) + f(d))) * 0.25f;
    const uint32_t h = __builtin_bit_cast(uint16_t, (_Float16)r);
    return r != r ? 0x7e00u : h;
}
// two halfs in a word
__device__ __forceinline__ uint32_t resolve_word(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return resolve_half(a & 0xffffu, b & 0xffffu, c & 0xffffu, d & 0xffffu) | (resolve_half(a >> 16, b >> 16, c >> 16, d >> 16) << 16);
}
__device__ __forceinline__ uint2 resolve_texel(uint2 a, uint2 b, uint2 c, uint2 d) {
    return make_uint2(resolve_word(a.x, b.x, c.x, d.x), resolve_word(a.y, b.y, c.y, d.y));
}

template <bool VEC4>
__global__ void __launch_bounds__(256) k_vrsaa_resolve(const PlaneArg lit, const PlaneArg out, uint32_t w, uint32_t row_begin, uint32_t row_end) {
    constexpr uint32_t PPT = VEC4 ? 4u : 1u;
    const uint64_t x0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * PPT;  // (w / PPT groups; VEC4: w is a multiple of 4)
    if (x0 >= w) return;
    for (uint64_t y = (uint64_t)row_begin + blockIdx.y; y < row_end; y += gridDim.y) {
        const uint8_t* up = lit.ptr + (size_t)(2 * y) * lit.pitch + (size_t)x0 * 16;
        const uint8_t* lo = up + lit.pitch;
        uint8_t* dst = const_cast<uint8_t*>(out.ptr) + (size_t)y * out.pitch + (size_t)x0 * 8;
        if constexpr (VEC4) {
            uint4 u[4], l[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                u[i] = reinterpret_cast<const uint4*>(up)[i];
                l[i] = reinterpret_cast<const uint4*>(lo)[i];
            }
            uint2 r[4];
#pragma unroll
            for (int i = 0; i < 4; i++)
                r[i] = resolve_texel(make_uint2(u[i].x, u[i].y), make_uint2(u[i].z, u[i].w), make_uint2(l[i].x, l[i].y), make_uint2(l[i].z, l[i].w));
            reinterpret_cast<uint4*>(dst)[0] = make_uint4(r[0].x, r[0].y, r[1].x, r[1].y);
            reinterpret_cast<uint4*>(dst)[1] = make_uint4(r[2].x, r[2].y, r[3].x, r[3].y);
        } else {
            const uint2* u = reinterpret_cast<const uint2*>(up);
            const uint2* l = reinterpret_cast<const uint2*>(lo);
            *reinterpret_cast<uint2*>(dst) = resolve_texel(u[0], u[1], l[0], l[1]);
        }
    }
}

}  // namespace

hipError_t launch_vrsaa_resolve(const PlaneArg& lit, const PlaneArg& out, uint32_t w, uint32_t h, uint32_t row_begin, uint32_t row_end, hipStream_t st) {
    (void)h;
    if (row_end <= row_begin || w == 0u) return hipSuccess;
    const bool vec4 = w % 4u == 0u && planes_aligned({&lit, &out}, 16);
    const uint32_t rows = row_end - row_begin, groups = vec4 ? w / 4u : w;
    const dim3 grid((groups + 255u) / 256u, rows < 65535u ? rows : 65535u);
    if (vec4) hipLaunchKernelGGL(k_vrsaa_resolve<true>, grid, dim3(256), 0, st, lit, out, w, row_begin, row_end);
    else hipLaunchKernelGGL(k_vrsaa_resolve<false>, grid, dim3(256), 0, st, lit, out, w, row_begin, row_end);
    return hipGetLastError();
}

}  // namespace sah
