// Variable-rate Lighting for gfx950 (include/sah_vrs.h): the shading-rate image of the VRSAA passes decides, per pixel, which pixel of the frame
// is shaded in its place — s(q), the representative of its coarse pixel or itself.  The kernel shades the pixels with s(q) = q, each with the
// general restatement at its own coordinates (lighting_common.hpp: exactly what sah_lighting computes there), and every pixel stores the bytes
// of its source.  No new shading arithmetic: a variable-rate frame is a gather of the full-rate frame.
//
// A kernel in which only the representatives' lanes shade would save nothing — the wave runs the whole body for one live lane as for 64.  The
// saving comes from compaction, workgroup by workgroup, with no cross-workgroup traffic:
//   256 threads own a region of 32 x 32 pixels: a multiple of every texel size up to 32, inside one texel at 64; its first row is a multiple of 4
//   (the row rule of the entry), so no coarse pixel crosses a region's edge.
//   1  the region's depths go to LDS; a thread owns four adjacent pixels of a row (inside one texel: texel sizes are multiples of 4), finds the
//      representative of each by scanning its coarse pixel in LDS and evaluates s(q);
//   2  the pixels with s(q) = q are compacted into an LDS list in row-major order: ballot + mbcnt per wave, wave totals through LDS (the idiom of
//      the tile culling in lighting_tiled.hip);
//   3  the list is dealt densely to the threads, shaded, the packed result put into an LDS tile;
//   4  every thread stores its four pixels from result[s(q)]: 32 contiguous bytes a thread.
// A region at 4 x 4 keeps one wave busy for one round where a region at 1 x 1 takes four rounds of all four.
#include <hip/hip_runtime.h>

#include "../../include/sah_vrs.h"
#include "launch.hpp"
#include "lighting_common.hpp"
#include "lighting_fast.hpp"
#include "numerics.hpp"
#include "params.hpp"

namespace sah {

constexpr uint32_t kVrsRegion = 32u;                      // pixels per side
constexpr uint32_t kVrsPixels = kVrsRegion * kVrsRegion;  // = 4 per thread
constexpr uint32_t kVrsNone = 0xffffu;

// LDS: 2 KB format tables + 4 KB depths + 2 KB list + 8 KB results = 16 KB
// Held at three waves per SIMD.  The shading loop wants 135-209 VGPRs (as k_lighting_fixup does: the restatement's uniform values outgrow the
// scalar registers): two waves per SIMD under an LPV, and at coarse rates — a round of shading or two per workgroup, most waves waiting at the
// barrier — the launch is bound by how many workgroups are resident.  At 168 VGPRs the LPV bodies spill 84-140 bytes a lane; measured at
// 3840 x 2160, CSM + LPV + sky (profiles/lighting_vrs_kernel_resources.txt): uniform 4 x 4 0.200 -> 0.166 ms, the library's own image 0.218 -> 0.184, 1 x 1
// 0.683 -> 0.626, 2 x 2 0.225 -> 0.229.  Four waves (128 VGPRs, 244-308 bytes) measured the same as three.
template <int SUN, int GI>
__global__ void __launch_bounds__(256, 3) k_lighting_vrs(const LightingArgs a, const CsmArgs csm, const LpvArgs lpv, const SkyArgs sky, const VrsArgs v) {
    __shared__ float s_lut[512];
    __shared__ __attribute__((aligned(16))) float s_depth[kVrsPixels];
    __shared__ uint16_t s_list[kVrsPixels];
    __shared__ uint2 s_result[kVrsPixels];
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x;
    stage_format_tables(s_lut, a.luts);

    const uint32_t rx0 = blockIdx.x * kVrsRegion, ry0 = a.row_begin + blockIdx.y * kVrsRegion;
    const uint32_t ly = tid >> 3, lx0 = (tid & 7u) * 4u;
    const uint32_t x0 = rx0 + lx0, y = ry0 + ly;
    const bool row_in = y < a.row_end;  // (row_end <= height)

    // ---- 1: depths (0 = no surface outside the image and the row range) and the thread's rate code
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t code = 0u;
    if (row_in && x0 < a.width) {
        const uint8_t* src = a.depth.ptr + (size_t)y * a.depth.pitch + (size_t)x0 * 4;
        if (v.vec4) {  // (uniform; the width is then a multiple of 4: all four pixels are inside)
            uint32_t w[4];
            load_words<4>(src, w);
#pragma unroll
            for (int i = 0; i < 4; i++) d[i] = __uint_as_float(w[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x0 + (uint32_t)i < a.width) d[i] = *reinterpret_cast<const float*>(src + 4 * i);
        }
        code = v.rate.ptr[(size_t)(y >> v.texel_shift[1]) * v.rate.pitch + (x0 >> v.texel_shift[0])];
    }
    *reinterpret_cast<float4*>(&s_depth[tid * 4u]) = make_float4(d[0], d[1], d[2], d[3]);
    __syncthreads();

    const uint32_t lw = min((code >> 2) & 3u, 2u), lh = min(code & 3u, 2u);
    const uint32_t cw = 1u << lw, ch = 1u << lh;
    const uint32_t cy = ly & ~(ch - 1u);
    uint32_t src_of[4];  // region-local index of s(q)
    uint32_t mine = 0u;  // bit i: pixel i is a shading point
    uint32_t r = kVrsNone;
    float dr = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t lx = lx0 + (uint32_t)i, q = ly * kVrsRegion + lx;
        if ((lx & (cw - 1u)) == 0u) {  // a new coarse pixel: its first surface pixel in row-major order (pixels cut off read 0)
            r = kVrsNone;
            for (uint32_t j = ch; j-- > 0u;)
                for (uint32_t k = cw; k-- > 0u;) {
                    const uint32_t at = (cy + j) * kVrsRegion + lx + k;
                    const float dv = s_depth[at];
                    if (dv != 0.f) {
                        r = at;
                        dr = dv;
                    }
                }
        }
        const float dq = d[i];
        const bool share = dq != 0.f && r != kVrsNone && __builtin_fabsf(dq - dr) <= v.depth_tolerance * __builtin_fabsf(dr);
        src_of[i] = share ? r : q;
        if (row_in && x0 + (uint32_t)i < a.width && src_of[i] == q) mine |= 1u << i;
    }
    const uint32_t src01 = src_of[0] | (src_of[1] << 16), src23 = src_of[2] | (src_of[3] << 16);

    // ---- 2: the shading points, compacted in row-major order (thread order, then the thread's four)
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t m = __ballot((mine >> i) & 1u);
        before += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        total += (uint32_t)__builtin_popcountll(m);
    }
    const uint32_t wave = tid >> 6;
    if ((tid & 63u) == 0u) s_wave[wave] = total;
    __syncthreads();
    uint32_t n = 0u, pos = before;
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) {
        const uint32_t t = s_wave[w];
        if (w < wave) pos += t;
        n += t;
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
        if ((mine >> i) & 1u) s_list[pos++] = (uint16_t)(ly * kVrsRegion + lx0 + (uint32_t)i);
    __syncthreads();

    // ---- 3: shade the list, densely (n is uniform over the workgroup; no barrier inside)
#pragma unroll 1
    for (uint32_t i = tid; i < n; i += 256u) {
        const uint32_t q = s_list[i];
        const uint32_t px = rx0 + (q & (kVrsRegion - 1u)), py = ry0 + (q >> 5);
        Px p;
        p.color = *reinterpret_cast<const uint32_t*>(a.color.ptr + (size_t)py * a.color.pitch + (size_t)px * 4);
        p.data = *reinterpret_cast<const uint32_t*>(a.data.ptr + (size_t)py * a.data.pitch + (size_t)px * 4);
        p.emission = *reinterpret_cast<const uint32_t*>(a.emission.ptr + (size_t)py * a.emission.pitch + (size_t)px * 4);
        p.depth = s_depth[q];
        const uint2 nn = *reinterpret_cast<const uint2*>(a.normals.ptr + (size_t)py * a.normals.pitch + (size_t)px * 8);
        p.n01 = nn.x;
        p.n23 = nn.y;
        p.ao = (GI == SAH_GI_LPV && a.has_ao) ? *reinterpret_cast<const float*>(a.ao.ptr + (size_t)py * a.ao.pitch + (size_t)px * 4) : 1.0f;
        p.mask = (SUN == SAH_SHADOW_MODE_RT && a.has_mask)
                     ? *reinterpret_cast<const float*>(a.shadow_mask.ptr + (size_t)py * a.shadow_mask.pitch + (size_t)px * 4)
                     : 1.0f;
        s_result[q] = shade_pixel_general<SUN, GI>(a, csm, lpv, sky, px, py, p, s_lut);
    }
    __syncthreads();

    // ---- 4: every pixel stores the bytes of its source
    if (!row_in || x0 >= a.width) return;
    const uint2 o0 = s_result[src01 & 0xffffu], o1 = s_result[src01 >> 16], o2 = s_result[src23 & 0xffffu], o3 = s_result[src23 >> 16];
    uint8_t* dst = const_cast<uint8_t*>(a.lit.ptr) + (size_t)y * a.lit.pitch + (size_t)x0 * 8;
    if (v.vec4) {
        const uint32_t out[8] = {o0.x, o0.y, o1.x, o1.y, o2.x, o2.y, o3.x, o3.y};
        store_words<8>(dst, out);
    } else {
        const uint2 o[4] = {o0, o1, o2, o3};
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (x0 + (uint32_t)i < a.width) *reinterpret_cast<uint2*>(dst + 8 * i) = o[i];
    }
}

template <int SUN>
static hipError_t launch_vrs_gi(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const SkyArgs& sky, const VrsArgs& v, int gi, dim3 grid,
                                hipStream_t st) {
    switch (gi) {
        case SAH_GI_NONE: hipLaunchKernelGGL((k_lighting_vrs<SUN, SAH_GI_NONE>), grid, dim3(256), 0, st, a, csm, lpv, sky, v); break;
        case SAH_GI_LPV: hipLaunchKernelGGL((k_lighting_vrs<SUN, SAH_GI_LPV>), grid, dim3(256), 0, st, a, csm, lpv, sky, v); break;
        default: return hipErrorNotSupported;
    }
    return hipGetLastError();
}

hipError_t launch_lighting_vrs(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const SkyArgs& sky, const VrsArgs& v, int sun_mode, int gi,
                               hipStream_t st) {
    const uint32_t rows = a.row_end - a.row_begin;
    if (rows == 0u || a.width == 0u) return hipSuccess;
    const uint32_t gx = (a.width + kVrsRegion - 1u) / kVrsRegion, gy = (rows + kVrsRegion - 1u) / kVrsRegion;
    if (gy > 65535u) return hipErrorInvalidValue;  // (2 M rows)
    const dim3 grid(gx, gy);
    switch (sun_mode) {
        case SAH_SHADOW_MODE_OFF: return launch_vrs_gi<SAH_SHADOW_MODE_OFF>(a, csm, lpv, sky, v, gi, grid, st);
        case SAH_SHADOW_MODE_CSM: return launch_vrs_gi<SAH_SHADOW_MODE_CSM>(a, csm, lpv, sky, v, gi, grid, st);
        case SAH_SHADOW_MODE_RT: return launch_vrs_gi<SAH_SHADOW_MODE_RT>(a, csm, lpv, sky, v, gi, grid, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace sah
