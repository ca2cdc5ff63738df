// The per-wave LPV texel box of the fast Lighting kernel (lighting.hip: k_lighting_fast with an LPV overlay; lighting_fast.hpp stages it and taps
// from it).  Integers only, host and device: the host restates nothing, tests/cpp/lpv_box_check.cpp compiles this very file.
//
// The gather copy (params.hpp: FastArgs::lpv_packed) holds P = size + 2 * border texels per axis, 24 bytes each.  A pixel's trilinear footprint is
// the 2 x 2 x 2 texels at its base (x0, y0, z0), each in [0, size + border] = [0, P - 2] (lighting_common.hpp: lpv_fetch_packed).  Neighbouring
// pixels share almost all of them, so a wave fetches one box of kLpvBoxEdge^3 texels around the base r of a reference lane once, widens it to fp32
// and keeps it in LDS:
//   origin   o = clamp(r - 1, 0, P - kLpvBoxEdge) per axis; the box is texels [o, o + kLpvBoxEdge)
//   served   base - o in [0, kLpvBoxEdge - 2] on all three axes: both taps of every axis are then inside the box
// In LDS a box texel is 48 bytes {R[4], G[4], B[4]} of fp32, x fastest, then y, then z (z slabs padded: kLpvBoxSlab): twice the byte offsets of the
// copy's 24-byte texel, so a 16-byte chunk of the copy becomes the 32 bytes at twice its offset inside its (y, z) row.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SAH_LPV_BOX_FN __host__ __device__ inline
#else
#define SAH_LPV_BOX_FN inline
#endif

namespace sah {

constexpr uint32_t kLpvBoxEdge = 4;                                              // texels per axis
constexpr uint32_t kLpvBoxSrcTexel = 24, kLpvBoxPad = 2;                         // the gather copy's texel and border (params.hpp: kLpvPackTexel, kLpvPackBorder)
constexpr uint32_t kLpvBoxTexel = 2 * kLpvBoxSrcTexel;                           // 48: an fp32 box texel
constexpr uint32_t kLpvBoxRow = kLpvBoxEdge * kLpvBoxTexel;                      // 192: one (y, z) row of the box in LDS
// A z slab of the box is 4 rows and 16 bytes of padding.  ds_read_b128 banks repeat every 256 bytes: unpadded, a slab is 768 bytes and two lanes
// whose bases differ on z alone read the same banks.  With 784 the offsets of lanes that differ on x and z are 16 * (3 dx + dz), all distinct.
constexpr uint32_t kLpvBoxSlab = kLpvBoxEdge * kLpvBoxRow + 16;                  // 784
constexpr uint32_t kLpvBoxBytes = kLpvBoxEdge * kLpvBoxSlab;                     // 3136 per wave
constexpr uint32_t kLpvBoxSrcRow = kLpvBoxEdge * kLpvBoxSrcTexel;                // 96 contiguous bytes of the copy per (y, z) row
constexpr uint32_t kLpvBoxChunksPerRow = kLpvBoxSrcRow / 16;                     // 6 chunks of 16 bytes
constexpr uint32_t kLpvBoxChunks = kLpvBoxEdge * kLpvBoxEdge * kLpvBoxChunksPerRow;  // 96: lane l stages chunks l and 64 + (l & 31)

// padded extent of an axis of `size` texels
SAH_LPV_BOX_FN uint32_t lpv_box_padded(uint32_t size) { return size + 2u * kLpvBoxPad; }

// box origin on one axis for the reference base r in [0, size + 2] (padded coordinates)
SAH_LPV_BOX_FN uint32_t lpv_box_origin(uint32_t r, uint32_t size) {
    const uint32_t hi = lpv_box_padded(size) - kLpvBoxEdge;
    const uint32_t lo = r == 0u ? 0u : r - 1u;
    return lo < hi ? lo : hi;
}

// a pixel's offset inside the box on one axis, and whether both taps of the axis are inside (base < o wraps to a large value: not served)
SAH_LPV_BOX_FN uint32_t lpv_box_delta(uint32_t base, uint32_t o) { return base - o; }
SAH_LPV_BOX_FN bool lpv_box_served(uint32_t dx, uint32_t dy, uint32_t dz) {
    return dx <= kLpvBoxEdge - 2u && dy <= kLpvBoxEdge - 2u && dz <= kLpvBoxEdge - 2u;
}
// the offset a lane uses: a lane that is not served (its result is discarded) still reads inside the box
SAH_LPV_BOX_FN uint32_t lpv_box_clamp_delta(uint32_t d) { return d < kLpvBoxEdge - 2u ? d : kLpvBoxEdge - 2u; }

// LDS byte offset, inside the wave's box, of the first tap (x0, y0, z0) of a pixel at (dx, dy, dz), each in [0, 2] ...
SAH_LPV_BOX_FN uint32_t lpv_box_lds_base(uint32_t dx, uint32_t dy, uint32_t dz) {
    return dz * kLpvBoxSlab + dy * kLpvBoxRow + dx * kLpvBoxTexel;
}
// ... and of the pixel's (y, z) row k = yy + 2 * zz (the order of lpv_fetch_packed: (y0,z0) (y1,z0) (y0,z1) (y1,z1)), 96 bytes: x0 then x1
SAH_LPV_BOX_FN uint32_t lpv_box_lds_row(uint32_t k) { return (k >> 1) * kLpvBoxSlab + (k & 1u) * kLpvBoxRow; }

// staged chunk c in [0, kLpvBoxChunks): byte offset in the gather copy for the origin (ox, oy, oz), and where its 32 widened bytes go
SAH_LPV_BOX_FN uint32_t lpv_box_chunk_src(uint32_t c, uint32_t ox, uint32_t oy, uint32_t oz, uint32_t row_pitch, uint32_t slice_pitch) {
    const uint32_t row = c / kLpvBoxChunksPerRow, j = c - row * kLpvBoxChunksPerRow;
    return (oz + row / kLpvBoxEdge) * slice_pitch + (oy + row % kLpvBoxEdge) * row_pitch + ox * kLpvBoxSrcTexel + 16u * j;
}
SAH_LPV_BOX_FN uint32_t lpv_box_chunk_dst(uint32_t c) {
    const uint32_t row = c / kLpvBoxChunksPerRow, j = c - row * kLpvBoxChunksPerRow;
    return (row / kLpvBoxEdge) * kLpvBoxSlab + (row % kLpvBoxEdge) * kLpvBoxRow + 32u * j;
}

// The reference lane of a slot: the first lane of `act` at or behind the lane at the centre of the wave's tile, else the last one before it
// (`act` != 0).  centre = (rows / 2) * lanes per row + lanes per row / 2 with 64 / ppt lanes per row and ppt rows: 40, 48, 32 at 4, 2, 1 pixels per
// thread.
SAH_LPV_BOX_FN uint32_t lpv_box_centre_lane(uint32_t ppt) { return (ppt / 2u) * (64u / ppt) + 32u / ppt; }
SAH_LPV_BOX_FN uint32_t lpv_box_reference_lane(uint64_t act, uint32_t centre) {
    const uint64_t behind = act & (~0ull << centre);
    return behind ? (uint32_t)__builtin_ctzll(behind) : 63u - (uint32_t)__builtin_clzll(act);
}

}  // namespace sah
