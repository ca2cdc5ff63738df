// Refit of the acceleration structure (include/sah_rt_refit.h): the triangles and the order of the last sah_rt_build stay, the
// coordinates are refreshed from the scene arrays as they are now.  A hit is defined through the triangle's own padded box
// (include/sah_hip.h "ray tracing"), so any hierarchy of enclosing boxes gives the build's results: a refit only has to make every box
// enclose its children again, and min / max do that exactly in any order.
//
//   k_rt_refit_world    one thread per structure position: new world vertices into the triangle record (ids and flag words kept), the
//                       UNPADDED box — or the absent box — into the position's lane of level 0, |coordinate| maximum and present /
//                       absent counts into RtBuildState with one atomic per wave
//   k_rt_refit_levels   a workgroup of 256 threads owns 256 consecutive nodes of its input level and with them, the hierarchy being
//                       implicit and complete, the 64 / 16 / 4 / 1 nodes of the four levels above.  The first launch turns level 0's
//                       unpadded boxes into padded ones (pad from DEVICE memory: the maximum the kernel before it reduced) and stores
//                       them; later launches start from the level the one before finished.  Two launches up to 65 536 triangles.
// pad = S * 2^-16 could not be applied by k_rt_refit_world (S is complete only when its last workgroup is), and a zeroed record cannot
// say "absent" (a triangle at the origin is all zeros too): level 0 itself carries the box between the two kernels.  (min - pad) of the
// stored min is tri_box's expression, the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.hpp"
#include "numerics.hpp"
#include "rt_args.hpp"
#include "rt_build_common.hpp"

namespace sah {
namespace {

constexpr float kInf = __builtin_inff();

__global__ __launch_bounds__(256) void k_rt_refit_world(const RtScene sc, RtTriangle* tris, uint32_t num_tris, RtNodeGroup* level0, RtBuildState* st) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool present = false;
    float amax = 0.f;
    if (i < num_tris) {
        float4* rec = reinterpret_cast<float4*>(tris + i);
        const uint32_t p = tris[i].primitive, tri = tris[i].triangle, flags = tris[i].flags;
        float v[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
        present = p < sc.num_primitives;  // (the build puts no left-out record below num_tris; a stray id must not leave the arrays)
        if (present) {
            const sah_primitive prim = sc.primitives[p];
            present = (uint64_t)prim.first_index + 3ull * tri + 2ull < (uint64_t)sc.num_indices;
            for (int k = 0; k < 3 && present; k++) {
                const int64_t vi = (int64_t)prim.vertex_offset + (int64_t)sc.indices[prim.first_index + 3u * tri + (uint32_t)k];
                present = vi >= 0 && vi < (int64_t)sc.num_vertices;
                if (!present) break;
                const float* pos = sc.positions + 3 * vi;
                for (int c = 0; c < 3; c++) v[k][c] = mat_row3(prim.model, c, pos[0], pos[1], pos[2]);
                present = finite3(v[k]);
            }
        }
        float lo[3], hi[3];
        for (int c = 0; c < 3; c++) {
            if (!present) v[0][c] = v[1][c] = v[2][c] = 0.f;
            lo[c] = present ? __builtin_fminf(__builtin_fminf(v[0][c], v[1][c]), v[2][c]) : kInf;
            hi[c] = present ? __builtin_fmaxf(__builtin_fmaxf(v[0][c], v[1][c]), v[2][c]) : kInf;
            if (present) amax = __builtin_fmaxf(amax, __builtin_fmaxf(__builtin_fabsf(lo[c]), __builtin_fabsf(hi[c])));
        }
        rec[0] = make_float4(v[0][0], v[0][1], v[0][2], __uint_as_float(p));
        rec[1] = make_float4(v[1][0], v[1][1], v[1][2], __uint_as_float(tri));
        rec[2] = make_float4(v[2][0], v[2][1], v[2][2], __uint_as_float(flags));
        RtNodeGroup& g = level0[i / kRtFanout];
        for (int c = 0; c < 3; c++) {
            g.lo[c][i % kRtFanout] = lo[c];
            g.hi[c][i % kRtFanout] = hi[c];
        }
    }
    // wave-aggregated statistics (k_rt_world's)
    const uint64_t mp = __ballot(present), ma = __ballot(i < num_tris);
    float wmax = amax;
    for (int d = 32; d >= 1; d >>= 1) wmax = __builtin_fmaxf(wmax, __shfl_xor(wmax, d, 64));
    if ((threadIdx.x & 63u) == 0 && ma) {
        const uint32_t np = (uint32_t)__builtin_popcountll(mp), na = (uint32_t)__builtin_popcountll(ma);
        if (np) {
            atomicAdd(&st->kept, np);
            atomicMax(&st->max_abs_bits, __float_as_uint(wmax));
        }
        if (na - np) atomicAdd(&st->dropped, na - np);
    }
}

struct RefitLevels {  // what one launch sees of RtBvh's level table: its input level ([0]) and the up to four levels above it
    uint32_t levels;     // how many of the five exist
    uint32_t offset[5], count[5];
};

// the values of one component in the four sibling lanes, in sibling order: slot = this lane's place among them, x1 / x2 / x3 what the
// lanes at slot ^ 1, ^ 2, ^ 3 hold
SAH_DEV float4 in_slot_order(float v, float x1, float x2, float x3, uint32_t slot) {
    const bool s1 = (slot & 1u) != 0u, s2 = (slot & 2u) != 0u;
    const float a0 = s1 ? x1 : v, a1 = s1 ? v : x1, a2 = s1 ? x3 : x2, a3 = s1 ? x2 : x3;
    return s2 ? make_float4(a2, a3, a0, a1) : make_float4(a0, a1, a2, a3);
}

// (selects on VALUES: a conditional expression on whole float4 objects goes through their addresses, and with them through scratch)
SAH_DEV float4 sel4(bool c, const float4& a, const float4& b) { return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w); }

// One level inside a wave.  Every lane holds the box of node (n / REP) of the level — REP consecutive lanes the same one — as it is
// STORED (an absent node: lo = hi = +inf; lo[0] == +inf says so, a present node's lo is min - pad of finite numbers).  The four siblings
// of a group sit REP lanes apart: three exchanges per component give every lane the group's six words, which `store` lanes write whole,
// and the parent — min / max over the present siblings, absent if there is none — replicated over 4 * REP lanes.
template <uint32_t REP>
SAH_DEV void wave_level(float lo[3], float hi[3], uint32_t lane, bool store, float4* group) {
    const uint32_t slot = (lane / REP) & 3u;
    float4 w[6];
    float plo[3], phi[3];
    const float l1 = __shfl_xor(lo[0], (int)REP, 64), l2 = __shfl_xor(lo[0], (int)(2u * REP), 64), l3 = __shfl_xor(lo[0], (int)(3u * REP), 64);
    const bool a0 = lo[0] == kInf, a1 = l1 == kInf, a2 = l2 == kInf, a3 = l3 == kInf;
    for (int c = 0; c < 3; c++) {
        const float x1 = c ? __shfl_xor(lo[c], (int)REP, 64) : l1, x2 = c ? __shfl_xor(lo[c], (int)(2u * REP), 64) : l2,
                    x3 = c ? __shfl_xor(lo[c], (int)(3u * REP), 64) : l3;
        const float y1 = __shfl_xor(hi[c], (int)REP, 64), y2 = __shfl_xor(hi[c], (int)(2u * REP), 64), y3 = __shfl_xor(hi[c], (int)(3u * REP), 64);
        w[c] = in_slot_order(lo[c], x1, x2, x3, slot);
        w[3 + c] = in_slot_order(hi[c], y1, y2, y3, slot);
        plo[c] = __builtin_fminf(__builtin_fminf(lo[c], x1), __builtin_fminf(x2, x3));  // an absent sibling's +inf is min's identity
        phi[c] = __builtin_fmaxf(__builtin_fmaxf(a0 ? -kInf : hi[c], a1 ? -kInf : y1), __builtin_fmaxf(a2 ? -kInf : y2, a3 ? -kInf : y3));
    }
    if (store) {
        const uint32_t cl = lane & (4u * REP - 1u);  // 4 * REP lanes hold the same six words
        if (REP == 1u) {
            group[cl] = sel4(cl < 2u, sel4(cl == 0u, w[0], w[1]), sel4(cl == 2u, w[2], w[3]));
            if (cl < 2u) group[4u + cl] = sel4(cl == 0u, w[4], w[5]);
        } else if (cl < 6u) {
            group[cl] = sel4(cl < 2u, sel4(cl == 0u, w[0], w[1]), sel4(cl < 4u, sel4(cl == 2u, w[2], w[3]), sel4(cl == 4u, w[4], w[5])));
        }
    }
    const bool none = a0 && a1 && a2 && a3;
    for (int c = 0; c < 3; c++) {
        lo[c] = plo[c];
        hi[c] = none ? kInf : phi[c];
    }
}

template <bool FIRST>
__global__ __launch_bounds__(256) void k_rt_refit_levels(RtNodeGroup* nodes, const RefitLevels t, const RtBuildState* st, uint32_t* stats) {
    __shared__ float s_box[4][6];
    const uint32_t n = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t count = t.count[0];
    float4* base = reinterpret_cast<float4*>(nodes);  // six words per group
    float lo[3] = {kInf, kInf, kInf}, hi[3] = {kInf, kInf, kInf};
    if (n < count) {
        const RtNodeGroup& g = nodes[t.offset[0] + n / kRtFanout];
        for (int c = 0; c < 3; c++) {
            lo[c] = g.lo[c][n % kRtFanout];
            hi[c] = g.hi[c][n % kRtFanout];
        }
        if (FIRST && lo[0] != kInf) {
            const float pad = __uint_as_float(st->max_abs_bits) * 0x1p-16f;
            for (int c = 0; c < 3; c++) {
                lo[c] -= pad;
                hi[c] += pad;
            }
        }
    }
    if (FIRST && n == 0u && stats) {
        stats[0] = st->kept;
        stats[1] = st->dropped;
        stats[2] = st->max_abs_bits;
        stats[3] = 0u;
    }
    // a group is stored when its first node exists; lanes of it that stand for no node hold the absent box already.  (k is a constant
    // at every use: the table stays in scalar registers)
#define SAH_REFIT_EXISTS(k, node) ((k) < t.levels && ((node) & ~3u) < t.count[k])
#define SAH_REFIT_GROUP(k, node) (base + 6ull * (t.offset[k] + (node) / kRtFanout))
    wave_level<1u>(lo, hi, lane, FIRST && SAH_REFIT_EXISTS(0, n), SAH_REFIT_GROUP(0, n));
    wave_level<4u>(lo, hi, lane, SAH_REFIT_EXISTS(1, n >> 2), SAH_REFIT_GROUP(1, n >> 2));
    wave_level<16u>(lo, hi, lane, SAH_REFIT_EXISTS(2, n >> 4), SAH_REFIT_GROUP(2, n >> 4));
    // level 3: one node per wave, the group of the workgroup's four through LDS
    if (lane == 0u)
        for (int c = 0; c < 3; c++) {
            s_box[threadIdx.x >> 6][c] = lo[c];
            s_box[threadIdx.x >> 6][3 + c] = hi[c];
        }
    __syncthreads();
    if (threadIdx.x < 6u && SAH_REFIT_EXISTS(3, n >> 6))
        SAH_REFIT_GROUP(3, n >> 6)[threadIdx.x] = make_float4(s_box[0][threadIdx.x], s_box[1][threadIdx.x], s_box[2][threadIdx.x], s_box[3][threadIdx.x]);
    // level 4: the workgroup's one node, a lane of a group that four workgroups share
    if (threadIdx.x == 0u && 4u < t.levels) {
        float plo[3] = {kInf, kInf, kInf}, phi[3] = {-kInf, -kInf, -kInf};
        bool none = true;
        for (uint32_t k = 0; k < kRtFanout; k++) {
            if (s_box[k][0] == kInf) continue;  // absent, or no such node
            none = false;
            for (int c = 0; c < 3; c++) {
                plo[c] = __builtin_fminf(plo[c], s_box[k][c]);
                phi[c] = __builtin_fmaxf(phi[c], s_box[k][3 + c]);
            }
        }
        const uint32_t m = blockIdx.x;
        RtNodeGroup& g = nodes[t.offset[4] + m / kRtFanout];
        for (int c = 0; c < 3; c++) {
            g.lo[c][m % kRtFanout] = plo[c];
            g.hi[c][m % kRtFanout] = none ? kInf : phi[c];
        }
        if (m + 1u == t.count[4]) fill_absent(g, t.count[4] % kRtFanout);
    }
#undef SAH_REFIT_EXISTS
#undef SAH_REFIT_GROUP
}

}  // namespace

// `st` must have kept, dropped and max_abs_bits zeroed on the stream before this
hipError_t launch_rt_refit(const RtScene& sc, const RtBvh& bvh, RtTriangle* tris, RtNodeGroup* nodes, RtBuildState* st, uint32_t* stats, hipStream_t s) {
    if (bvh.num_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rt_refit_world, dim3((bvh.num_tris + 255u) / 256u), dim3(256), 0, s, sc, tris, bvh.num_tris, nodes, st);
    // level `first` is finished when a launch starts from it; it is the top when first + 1 == num_levels
    for (uint32_t first = 0; first == 0 || first + 1u < bvh.num_levels; first += 4) {
        RefitLevels t = {};
        t.levels = bvh.num_levels - first < 5u ? bvh.num_levels - first : 5u;
        for (uint32_t k = 0; k < t.levels; k++) {
            t.offset[k] = bvh.level_offset[first + k];
            t.count[k] = bvh.level_count[first + k];
        }
        const dim3 grid((t.count[0] + 255u) / 256u);
        if (first == 0) hipLaunchKernelGGL(k_rt_refit_levels<true>, grid, dim3(256), 0, s, nodes, t, st, stats);
        else hipLaunchKernelGGL(k_rt_refit_levels<false>, grid, dim3(256), 0, s, nodes, t, st, stats);
    }
    return hipGetLastError();
}

}  // namespace sah
