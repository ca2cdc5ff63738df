// What the build (rt.hip) and the refit (rt_refit.hip) of the acceleration structure both do per triangle and per node group: the vertex
// transform, the finiteness test, the padded box, the box of a lane that stands for no node.  One statement of each, so that a refit
// gives the build's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "numerics.hpp"
#include "rt_args.hpp"

namespace sah {

SAH_DEV bool finite3(const float v[3]) {
    return __builtin_fabsf(v[0]) < __builtin_inff() && __builtin_fabsf(v[1]) < __builtin_inff() && __builtin_fabsf(v[2]) < __builtin_inff();
}

SAH_DEV float mat_row3(const float* m, int r, float x, float y, float z) { return ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r]; }

SAH_DEV void tri_box(const RtTriangle& r, float pad, float lo[3], float hi[3]) {
    for (int c = 0; c < 3; c++) {
        lo[c] = __builtin_fminf(__builtin_fminf(r.v0[c], r.v1[c]), r.v2[c]) - pad;
        hi[c] = __builtin_fmaxf(__builtin_fmaxf(r.v0[c], r.v1[c]), r.v2[c]) + pad;
    }
}

// The lanes of a level's last group that stand for no node hold the box [+inf, +inf]^3, which no ray passes: RN((+inf - o) * inv) is
// +inf on both planes of an axis where inv > 0 (entry = +inf > exit = min(tmax, +inf): make_ray keeps tmax FINITE, and the closest-hit
// walk only ever lowers it) and -inf where inv < 0 (exit = -inf < entry); inv is never 0 or NaN for a ray that walks (non-finite rays do
// not).  The walk then needs no "does this child exist" test.
SAH_DEV void fill_absent(RtNodeGroup& g, uint32_t first_absent) {
    if (first_absent == 0u) return;  // the group is full
    for (uint32_t k = first_absent; k < kRtFanout; k++)
        for (int c = 0; c < 3; c++) g.lo[c][k] = g.hi[c][k] = __builtin_inff();
}

}  // namespace sah
