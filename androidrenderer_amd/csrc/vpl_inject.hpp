// The vertex and fragment stage of vpl_injection.{vert,frag} (one light into one cascade) and the in-workgroup bitonic sort of up to
// 4096 (cell, sequence index) keys, shared by sah_lpv_inject_vpls (vpl.hip) and sah_lpv_inject_emissive (lpv_mesh_lights.hip).
// Arithmetic: GLSL fp32, every operator rounded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "numerics.hpp"
#include "params.hpp"
#include "../../include/sah_hip.h"

namespace sah {

SAH_DEV void mat_vec4(const float* m, float x, float y, float z, float w, float out[4]) {
    for (int r = 0; r < 4; r++) out[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w;
}

struct Injected {
    float sh[4];
    float corrected[3];
};
SAH_DEV float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }
SAH_DEV float stepf(float edge, float x) { return x < edge ? 0.0f : 1.0f; }
SAH_DEV float fractf(float x) { return x - __builtin_floorf(x); }
SAH_DEV float snorm8(uint32_t b) { return __builtin_fmaxf((float)(int8_t)(uint8_t)b / 127.0f, -1.0f); }

// vertex + fragment stage of one light; returns its cell (x + W (y + H z)) or ~0
template <class A> SAH_DEV uint32_t inject_one(const A& a, const sah_packed_vpl& p, Injected& out) {
    const float position[3] = {h2f((uint16_t)p.data[0]), h2f((uint16_t)(p.data[0] >> 16)), h2f((uint16_t)p.data[1])};
    const float color[3] = {h2f((uint16_t)(p.data[1] >> 16)), h2f((uint16_t)p.data[2]), h2f((uint16_t)(p.data[2] >> 16))};
    float normal[3] = {snorm8(p.data[3]), snorm8(p.data[3] >> 8), snorm8(p.data[3] >> 16)};
    const float inv = 1.0f / __builtin_sqrtf((normal[0] * normal[0] + normal[1] * normal[1]) + normal[2] * normal[2]);
    for (int k = 0; k < 3; k++) normal[k] = normal[k] * inv;
    float cp[4];
    mat_vec4(a.world_to_cascade, position[0], position[1], position[2], 1.0f, cp);
    const float px = (cp[0] + a.cascade_f) / a.num_cascades_f;
    const float ndc_x = px * 2.0f - 1.0f, ndc_y = cp[1] * 2.0f - 1.0f, layer_f = cp[2] * 32.0f;
    const float len_n = __builtin_sqrtf((normal[0] * normal[0] + normal[1] * normal[1]) + normal[2] * normal[2]);
    const float len_c = __builtin_sqrtf((color[0] * color[0] + color[1] * color[1]) + color[2] * color[2]);
    if (len_n < 1.0f || len_c == 0.0f) return ~0u;
    const float W = (float)a.rgb[0].width, H = (float)a.rgb[0].height, D = (float)a.rgb[0].depth;
    const float xf = ndc_x * (W * 0.5f) + W * 0.5f, yf = ndc_y * (H * 0.5f) + H * 0.5f;
    if (!(xf >= 0.0f && xf < W && yf >= 0.0f && yf < H)) return ~0u;
    if (!(layer_f > -1.0f && layer_f < D)) return ~0u;
    const uint32_t cx = (uint32_t)__builtin_floorf(xf), cy = (uint32_t)__builtin_floorf(yf), cz = (uint32_t)(int)layer_f;
    float scaled[3];
    for (int k = 0; k < 3; k++) scaled[k] = color[k] * 1024.0f / 16384.0f;
    const float Kx = 0.0f, Ky = -1.0f / 3.0f, Kz = 2.0f / 3.0f, Kw = -1.0f;
    const float s1 = stepf(scaled[2], scaled[1]);
    const float p4[4] = {mixf(scaled[2], scaled[1], s1), mixf(scaled[1], scaled[2], s1), mixf(Kw, Kx, s1), mixf(Kz, Ky, s1)};
    const float s2 = stepf(p4[0], scaled[0]);
    const float q4[4] = {mixf(p4[0], scaled[0], s2), mixf(p4[1], p4[1], s2), mixf(p4[3], p4[2], s2), mixf(scaled[0], p4[0], s2)};
    const float d = q4[0] - __builtin_fminf(q4[3], q4[1]);
    const float e = 1.0e-10f;
    float hsv[3] = {__builtin_fabsf(q4[2] + (q4[3] - q4[1]) / (6.0f * d + e)), d / (q4[0] + e), q4[0]};
    hsv[1] = hsv[1] * 2.0f;
    const float k4[4] = {1.0f, 2.0f / 3.0f, 1.0f / 3.0f, 3.0f};
    for (int k = 0; k < 3; k++) {
        const float pk = __builtin_fabsf(fractf(hsv[0] + k4[k]) * 6.0f - k4[3]);
        out.corrected[k] = hsv[2] * mixf(k4[0], __builtin_fminf(__builtin_fmaxf(pk - k4[0], 0.0f), 1.0f), hsv[1]);
    }
    const float c0 = 0.886226925f, c1 = 1.02332671f;
    out.sh[0] = c0; out.sh[1] = -c1 * normal[1]; out.sh[2] = c1 * normal[2]; out.sh[3] = -c1 * normal[0];
    return cx + a.rgb[0].width * (cy + a.rgb[0].height * cz);
}

constexpr uint32_t kSortCapacity = 4096;
// Bitonic network over 4096 keys held four per thread (key r of thread t is element r * 1024 + t), so that only the exchanges between
// waves go through LDS: partners 1024 or 2048 apart are two registers of one thread, partners less than 64 apart are two lanes of one
// wave (a shuffle), and the distances in between (64 .. 512: 18 of the 78 stages) take one LDS round trip each, ping-ponging two
// buffers.  As plain LDS compare-exchanges with a barrier per stage the sort was 120 of the kernel's 165 us.
SAH_DEV unsigned long long exch(unsigned long long x, unsigned long long y, bool keep_min) { return ((x < y) == keep_min) ? x : y; }
// Sorts key[0..3] of every thread of a 1024-thread workgroup (element r * 1024 + t); returns the LDS buffer that holds the 4096 sorted
// keys (not yet written: the caller stores key[r] to it at r * 1024 + t and synchronises).
SAH_DEV unsigned long long* bitonic_sort_4096(unsigned long long key[4], unsigned long long (*s_buf)[kSortCapacity]) {
    const uint32_t t = threadIdx.x;
    uint32_t flip = 0;
    for (uint32_t k = 2; k <= kSortCapacity; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (j >= 1024u) {  // rows of one thread: (0,1)(2,3) for j = 1024, (0,2)(1,3) for j = 2048
                const uint32_t d = j >> 10;
#pragma unroll
                for (uint32_t r = 0; r < 4; r++) {
                    if (r & d) continue;
                    const bool ascending = (((r * 1024u + t) & k) == 0u);
                    const unsigned long long x = key[r], y = key[r | d];
                    key[r] = exch(x, y, ascending);
                    key[r | d] = exch(y, x, !ascending);  // the other one (keys are distinct: the index is part of them)
                }
            } else if (j < 64u) {  // lanes of one wave
#pragma unroll
                for (uint32_t r = 0; r < 4; r++) {
                    const uint32_t i = r * 1024u + t;
                    const unsigned long long y = __shfl_xor(key[r], (int)j, 64);
                    const bool ascending = (i & k) == 0u, lower = (i & j) == 0u;
                    key[r] = exch(key[r], y, lower == ascending);
                }
            } else {  // other waves: one LDS round trip
                unsigned long long* buf = s_buf[flip];
                flip ^= 1u;
#pragma unroll
                for (uint32_t r = 0; r < 4; r++) buf[r * 1024u + t] = key[r];
                __syncthreads();
#pragma unroll
                for (uint32_t r = 0; r < 4; r++) {
                    const uint32_t i = r * 1024u + t;
                    const unsigned long long y = buf[i ^ j];
                    const bool ascending = (i & k) == 0u, lower = (i & j) == 0u;
                    key[r] = exch(key[r], y, lower == ascending);
                }
            }
        }
    }
    return s_buf[flip];
}

}  // namespace sah
