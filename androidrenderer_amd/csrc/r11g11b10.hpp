// B10G11R11_UFLOAT_PACK32 <-> fp16: the one decoder and encoder of every kernel that loads or stores the format (probes.hip, mip_chain.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "numerics.hpp"

namespace sah {

// ---- B10G11R11 <-> fp16 ---------------------------------------------------------------------------------------------------
// decode: uf11 = fp16 >> 4, uf10 = fp16 >> 5 (same exponent width and bias).  encode (float -> uf11/uf10): round toward zero,
// negatives -> 0, NaN -> canonical NaN, values above the largest finite -> largest finite (the choice documented in DESIGN.md §3).
SAH_DEV uint32_t f32_to_uf(float f, uint32_t mant_bits) {  // mant_bits = 6 (uf11) or 5 (uf10)
    const uint32_t x = __float_as_uint(f);
    const uint32_t exp_all = 0x1fu << mant_bits;
    if ((x & 0x7fffffffu) > 0x7f800000u) return exp_all | (1u << (mant_bits - 1));  // NaN
    if (x & 0x80000000u) return 0u;                                                // negative (incl. -inf, -0)
    if (x >= 0x7f800000u) return exp_all;                                          // +inf
    const uint32_t max_finite = exp_all - 1u;                                      // 0x7bf / 0x3df
    const uint32_t max_f32 = ((30u + 112u) << 23) | (((1u << mant_bits) - 1u) << (23u - mant_bits));
    if (x > max_f32) return max_finite;
    if (x < 0x38800000u) {  // below 2^-14: denormal in the small format, unit 2^-(14 + mant_bits)
        const uint32_t e = x >> 23;
        const uint32_t sh = (mant_bits == 6u ? 130u : 131u) - e;  // value = m * 2^(e - 150), unit 2^-20 (uf11) / 2^-19 (uf10)
        if (sh > 24u) return 0u;
        const uint32_t m = (x & 0x7fffffu) | 0x800000u;
        return m >> sh;
    }
    return (((x >> 23) - 112u) << mant_bits) | ((x & 0x7fffffu) >> (23u - mant_bits));
}
SAH_DEV uint32_t encode_r11g11b10(Hn r, Hn g, Hn b) { return f32_to_uf(tof(r), 6u) | (f32_to_uf(tof(g), 6u) << 11) | (f32_to_uf(tof(b), 5u) << 22); }
SAH_DEV void decode_r11g11b10(uint32_t w, Hn (&o)[3]) {
    o[0] = Hn::raw(__builtin_bit_cast(_Float16, (uint16_t)((w & 0x7ffu) << 4)));
    o[1] = Hn::raw(__builtin_bit_cast(_Float16, (uint16_t)(((w >> 11) & 0x7ffu) << 4)));
    o[2] = Hn::raw(__builtin_bit_cast(_Float16, (uint16_t)(((w >> 22) & 0x3ffu) << 5)));
}
// a texel that goes through `half3 t = src[..]; dst[..] = t;`: every bit pattern survives except NaNs, which become the canonical one
SAH_DEV uint32_t roundtrip_r11g11b10(uint32_t w) {
    Hn c[3];
    decode_r11g11b10(w, c);
    return encode_r11g11b10(c[0], c[1], c[2]);
}

}  // namespace sah
