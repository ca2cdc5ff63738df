// Histogram auto-exposure for gfx950 (include/sah_exposure.h): builder-owned arithmetic, restated by tests/exposure_ref.py.
//
// k_exposure_meter<kApply, kWide>: a persistent grid of 256-thread workgroups loops over 128 x 4 pixel tiles.  A wave takes one row of a
// tile — 128 adjacent pixels, 1 KB — and a lane two adjacent pixels of it: one 16-byte load on the wide path (every plane's pointer and
// pitch a multiple of 16), dwords otherwise; a row that ends on an odd width leaves its last lane one pixel.  With kApply the same lane
// stores the exposed pixels, so `exposed_out` may be `scene` itself.  Each wave keeps its own 256-bin sub-histogram in LDS and adds to it
// with non-returning LDS adds; a lane whose two pixels share a bin adds 2 once.  At the end of its loop a workgroup sums its four
// sub-histograms and adds its non-zero bins to the histogram in `work` with relaxed agent-scope atomics.
//
// Cross-workgroup hand-over (the ticket of mip_chain.hip's exit): every wave waits for its own atomics, the workgroup meets at a barrier,
// thread 0 releases at agent scope and then draws a ticket from work[256], and the workgroup that draws the last one acquires at agent
// scope and reads the 256 words with agent-scope atomic loads (the XCDs' L2s are not coherent: a plain load may be stale).  It forms the window
// and S in integers — a prefix sum over the bins through LDS, any arrangement of which gives the same bits — and thread 0 alone does the
// handful of fp32 operations and writes the state with ordinary stores.  `work` is zeroed ahead of every launch by k_exposure_clear, a
// kernel of this file and not hipMemsetAsync: a captured memset node was seen to write a stale 16-byte pattern instead of zeros from its
// second replay on (ROCm 7.2, any size from 4 bytes up), and a ticket word that is not zero means no workgroup ever draws the last ticket.
//
// k_exposure_apply<kWide>: the same lane map over a row window, one workgroup per tile.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "screen_common.hpp"

namespace sah {

constexpr int kExW = 128, kExH = 4;                // the tile: a wave per row, two pixels per lane
// The library's choice of grid: one workgroup per CU up to kExSmallTiles tiles, two beyond.  Every workgroup ends with up to 256 global
// atomics, a release and a ticket on one word, so more workgroups cost more than they hide: metering alone at 1280 x 720 / 3840 x 2160
// took 0.0144 / 0.0459 ms under 256 workgroups, 0.0181 / 0.0372 under 512, 0.0300 / 0.0420 under 1,024 and 0.0484 / 0.0627 under 2,048.
constexpr uint32_t kExSmallGrid = 256, kExLargeGrid = 512, kExSmallTiles = 4096;

namespace {

SAH_DEV uint32_t ex_f2u(float x) { return x >= 4294967296.0f ? 0xffffffffu : (x > 0.0f ? (uint32_t)x : 0u); }

// the bin of the pixel (lo = r | g << 16, hi = b | a << 16), or -1 when it is not counted
SAH_DEV int ex_bin(uint32_t lo, uint32_t hi) {
    const float r = half_lo(lo), g = half_hi(lo), b = half_lo(hi);
    const float L = (r * 0.2126f + g * 0.7152f) + b * 0.0722f;
    if (!(L > 0.0f && L < kScreenInf)) return -1;
    const int k = (int)(__builtin_bit_cast(uint32_t, L) >> 20) - 856;
    return k < 0 ? 0 : (k > 255 ? 255 : k);
}

SAH_DEV void ex_scale(uint32_t& lo, uint32_t& hi, float e) {
    const float r = half_lo(lo), g = half_hi(lo), b = half_lo(hi);
    lo = (uint32_t)f2h(r * e) | ((uint32_t)f2h(g * e) << 16);  // (not pack_half2: each product is rounded before the next is formed)
    hi = (uint32_t)f2h(b * e) | (hi & 0xffff0000u);
}

SAH_DEV void ex_count(uint32_t* hist, int k0, int k1) {
    if (k0 >= 0 && k0 == k1) {
        (void)__hip_atomic_fetch_add(hist + k0, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
    if (k0 >= 0) (void)__hip_atomic_fetch_add(hist + k0, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k1 >= 0) (void)__hip_atomic_fetch_add(hist + k1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The two pixels (x, y) and (x + 1, y) of a lane, x even; the second only where it lies inside the image.  kMeter: counted into `hist`;
// kApply: scaled by e into `out` (which may be `scene`: a lane reads its pixels before it writes them, and nobody else's).
template <bool kMeter, bool kApply, bool kWide>
SAH_DEV void ex_lane(const PlaneArg& scene, const PlaneArg& out, uint32_t W, uint32_t x, uint32_t y, float e, uint32_t* hist) {
    const uint8_t* src = scene.ptr + (size_t)y * scene.pitch + (size_t)x * 8;
    uint8_t* dst = const_cast<uint8_t*>(out.ptr) + (size_t)y * out.pitch + (size_t)x * 8;
    if (x + 1 < W) {
        uint4 v;
        if (kWide) {
            v = *reinterpret_cast<const uint4*>(src);
        } else {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
            v = make_uint4(s[0], s[1], s[2], s[3]);
        }
        if (kMeter) ex_count(hist, ex_bin(v.x, v.y), ex_bin(v.z, v.w));
        if (kApply) {
            ex_scale(v.x, v.y, e);
            ex_scale(v.z, v.w, e);
            if (kWide) {
                *reinterpret_cast<uint4*>(dst) = v;
            } else {
                uint32_t* d = reinterpret_cast<uint32_t*>(dst);
                d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
            }
        }
    } else {  // the single-pixel tail of an odd width
        const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
        uint32_t lo = s[0], hi = s[1];
        if (kMeter) ex_count(hist, ex_bin(lo, hi), -1);
        if (kApply) {
            ex_scale(lo, hi, e);
            uint32_t* d = reinterpret_cast<uint32_t*>(dst);
            d[0] = lo, d[1] = hi;
        }
    }
}

template <bool kApply, bool kWide> __global__ void __launch_bounds__(256) k_exposure_meter(ExposureArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[4][SAH_EXPOSURE_BINS];  // a sub-histogram per wave: 4 KB
    __shared__ uint32_t s_ticket;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
#pragma unroll
    for (int w = 0; w < 4; w++) s_hist[w][tid] = 0u;
    __syncthreads();
    const float e = kApply ? a.state_in->exposure : 0.0f;
    for (uint32_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
        const uint32_t x = tx * kExW + 2u * lane, y = ty * kExH + wave;
        if (x < a.W && y < a.H) ex_lane<true, kApply, kWide>(a.scene, a.out, a.W, x, y, e, s_hist[wave]);
    }
    __syncthreads();
    const uint32_t mine = (s_hist[0][tid] + s_hist[1][tid]) + (s_hist[2][tid] + s_hist[3][tid]);
    if (mine) (void)__hip_atomic_fetch_add(a.work + tid, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // The last workgroup to sign the ticket word goes on.  Every wave waits for its own adds (vmcnt(0): agent-scope atomics are performed
    // beyond the XCD's L2, so a completed add is visible chip-wide), the workgroup meets, and ONE lane releases at agent scope and then
    // draws the ticket: one L2 write-back per workgroup, not one per wave (five per workgroup cost 0.045 ms at 1,024 workgroups).  The
    // histogram does not depend on that write-back (its words are written by atomics alone), so it does not matter that the compiler,
    // seeing this wave's counter already waited for, leaves out the wait between the write-back and the ticket.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), the other counters left alone
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        s_ticket = __hip_atomic_fetch_add(a.work + SAH_EXPOSURE_BINS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s_ticket != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

    // Window: thread b holds n[b]; an inclusive prefix sum of n[1..255] through LDS (integers: any arrangement gives the same bits)
    const uint32_t n_b = tid ? __hip_atomic_load(a.work + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    uint32_t* scan = s_hist[0];                                                     // (the sub-histograms have been summed: their LDS is free)
    unsigned long long* s_sum = reinterpret_cast<unsigned long long*>(s_hist[2]);  // 256 x 8 bytes: the last two
    uint32_t incl = n_b;
    scan[tid] = incl;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < SAH_EXPOSURE_BINS; d <<= 1) {
        const uint32_t other = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        incl += other;
        scan[tid] = incl;
        __syncthreads();
    }
    const uint32_t N = scan[SAH_EXPOSURE_BINS - 1];
    const uint32_t lo_u = ex_f2u((float)N * a.low_fraction), hi_u = ex_f2u((float)N * a.high_fraction);
    const uint32_t lo = lo_u < N ? lo_u : N, hi = hi_u < N ? hi_u : N;
    const uint32_t C = incl - n_b;
    const auto cl = [lo, hi](uint32_t v) {
        const uint32_t m = v > lo ? v : lo;
        return m < hi ? m : hi;
    };
    const uint32_t c_b = cl(incl) - cl(C);  // (bin 0: n_b = 0, so 0)
    s_sum[tid] = (unsigned long long)c_b * (unsigned long long)(2u * tid + 1u);
    __syncthreads();
#pragma unroll
    for (uint32_t d = SAH_EXPOSURE_BINS / 2; d > 0; d >>= 1) {
        if (tid < d) s_sum[tid] += s_sum[tid + d];
        __syncthreads();
    }
    if (tid != 0) return;
    const unsigned long long S = s_sum[0];
    const bool metered = hi > lo;
    float m_p = 0.0f;
    bool history = false;
    if (a.history) {
        m_p = a.state_in->adapted;
        history = __builtin_fabsf(m_p) < kScreenInf;
    }
    float m = 0.0f;
    if (metered) {
        const float m_t = ((float)S / (float)(hi - lo)) * 0.0625f - 20.0f;
        m = history ? m_p + (m_t - m_p) * a.adaptation : m_t;
    } else {
        m = m_p;
    }
    sah_exposure_state out;
    if (metered || history) {
        const float L_avg = __builtin_bit_cast(float, ex_f2u((m + 127.0f) * 8388608.0f));
        out.exposure = sel_min(sel_max(a.key / L_avg, a.min_exposure), a.max_exposure);
        out.adapted = m;
    } else {
        out.exposure = sel_min(sel_max(1.0f, a.min_exposure), a.max_exposure);
        out.adapted = __builtin_bit_cast(float, 0x7fc00000u);
    }
    out.metered = N, out.window = hi - lo;
    *a.state_out = out;
}

__global__ void __launch_bounds__(320) k_exposure_clear(uint32_t* work) {
    if (threadIdx.x < SAH_EXPOSURE_WORK_BYTES / 4) work[threadIdx.x] = 0u;
}

template <bool kWide> __global__ void __launch_bounds__(256) k_exposure_apply(ExposureArgs a) {
    const uint32_t tid = threadIdx.x;
    const uint32_t ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const uint32_t x = tx * kExW + 2u * (tid & 63u), y = a.row_begin + ty * kExH + (tid >> 6);
    if (x >= a.W || y >= a.row_end) return;
    ex_lane<false, true, kWide>(a.scene, a.out, a.W, x, y, a.state_in->exposure, nullptr);
}

bool ex_wide(const ExposureArgs& a, bool with_out) {
    return planes_aligned({&a.scene}, 16) && (!with_out || planes_aligned({&a.out}, 16));
}

}  // namespace

hipError_t launch_exposure_meter(const ExposureArgs& in, bool apply, uint32_t max_workgroups, hipStream_t st) {
    ExposureArgs a = in;
    a.tiles_x = (a.W + kExW - 1) / kExW;
    a.tiles = a.tiles_x * ((a.H + kExH - 1) / kExH);  // (W * H < 2^32: fits)
    const uint32_t cap = max_workgroups ? max_workgroups : (a.tiles <= kExSmallTiles ? kExSmallGrid : kExLargeGrid);
    const uint32_t grid = a.tiles < cap ? a.tiles : cap;
    static_assert(SAH_EXPOSURE_WORK_BYTES / 4 <= 320, "one workgroup clears work");
    hipLaunchKernelGGL(k_exposure_clear, dim3(1), dim3(320), 0, st, a.work);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const bool wide = ex_wide(a, apply);
    void (*kernel)(ExposureArgs) = k_exposure_meter<false, false>;
    if (apply)
        kernel = wide ? k_exposure_meter<true, true> : k_exposure_meter<true, false>;
    else if (wide)
        kernel = k_exposure_meter<false, true>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_exposure_apply(const ExposureArgs& in, hipStream_t st) {
    if (in.row_end <= in.row_begin) return hipSuccess;
    ExposureArgs a = in;
    a.tiles_x = (a.W + kExW - 1) / kExW;
    a.tiles = a.tiles_x * ((a.row_end - a.row_begin + kExH - 1) / kExH);
    const dim3 grid(a.tiles);  // one dimension: no limit of 65535 tile rows
    hipLaunchKernelGGL(ex_wide(a, true) ? k_exposure_apply<true> : k_exposure_apply<false>, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sah
