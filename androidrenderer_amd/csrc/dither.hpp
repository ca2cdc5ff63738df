// The 4 x 4 ordered-dither matrix the screen-space passes share (include/sah_ssr.h states it; sah_motion_blur.h and sah_sun_shafts.h refer
// to it): one definition, so that the passes cannot drift apart.
#pragma once
#include <stdint.h>

#include "numerics.hpp"

namespace sah {

// the entry at [y & 3][x & 3], 0..15, as the float every pass scales by 1 / 16
SAH_DEV float bayer4x4(uint32_t x, uint32_t y) {
    constexpr float kBayer[16] = {0.f, 8.f, 2.f, 10.f, 12.f, 4.f, 14.f, 6.f, 3.f, 11.f, 1.f, 9.f, 15.f, 7.f, 13.f, 5.f};
    return kBayer[(x & 3u) + 4u * (y & 3u)];
}

}  // namespace sah
