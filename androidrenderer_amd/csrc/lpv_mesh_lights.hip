// LPV mesh lights (include/sah_lpv_mesh_lights.h): the point cloud of a mesh (host), the VPLs of an emissive primitive's cloud, and the
// per-frame injection of every selected cloud into every cascade.
//
// The injection is the point draw of vpl_injection.{vert,frag} with additive blending, so its result is a chain of half roundings per
// cell in (cascade, cloud, point) order.  Small calls (at most kSortCapacity entries, at most kChunk clouds: the atrium's 8 lamps x 5
// points x 4 cascades = 160) take one workgroup that sorts (cell, sequence index) keys in LDS, as sah_lpv_inject_vpls does.  Larger ones:
//   1. evaluate   one thread per entry (one launch per kChunk clouds, whose records travel as kernel arguments): selection, vertex stage,
//                 cell key (kDropped when the light is not drawn) and where its VPL lives;
//   2. sort       an LSD radix sort of the 18-bit keys, three passes of 6 bits (histogram per tile, one scan, stable scatter): it is
//                 stable, and the entries start in sequence order, so every cell ends up as one run in sequence order;
//   3. terms      the 12 blend sources of every kept entry, in parallel, stored in sorted order;
//   4. walk       the thread at the head of each run adds the run onto its texel, one rounding to half per add (serial by contract).
// The grids come from the host-known counts: nothing is read back and the call records under stream capture.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/sah_lpv_mesh_lights.h"
#include "ctx.hpp"
#include "numerics.hpp"
#include "params.hpp"
#include "texture_sample.hpp"
#include "vpl_inject.hpp"

namespace sah {
namespace {

// ---- VPLs of one primitive's cloud (emissive_point_cloud.comp) ----------------------------------------------------------------------
struct EmissiveArgs {
    const float* luts;
    const sah_primitive* primitives;
    const sah_material* materials;
    const sah_material_textures* material_textures;  // NULL: constant texels only
    const sah_texture* textures;
    uint32_t num_materials, num_textures, primitive, flags, num_points;
    const float* positions;
    const sah_vertex_data* points;
    sah_packed_vpl* out;
};

SAH_DEV uint32_t pack_half2(float lo, float hi) { return (uint32_t)f2h(lo) | ((uint32_t)f2h(hi) << 16); }

__global__ __launch_bounds__(256) void k_emissive_vpls(const EmissiveArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.num_points) return;
    const sah_primitive& prim = a.primitives[a.primitive];
    const uint32_t mi = (a.flags & SAH_EMISSIVE_MATERIAL_ZERO) ? 0u : prim.material;
    const sah_vertex_data& v = a.points[i];
    float color[3] = {0.0f, 0.0f, 0.0f};
    if (mi < a.num_materials) {
        const sah_material& mat = a.materials[mi];
        float s[4] = {mat.emission_texel[0], mat.emission_texel[1], mat.emission_texel[2], mat.emission_texel[3]};
        const uint32_t slot = a.material_textures ? a.material_textures[mi].emission : SAH_TEXTURE_NONE;
        if (slot != SAH_TEXTURE_NONE && slot < a.num_textures) {
            const sah_texture& T = a.textures[slot];
            if (T.num_mips >= 1 && T.num_mips <= SAH_MAX_TEXTURE_MIPS) {
                const float uv[2] = {v.texcoord[0], v.texcoord[1]};
                sample_texture_lod(a.luts, T, uv, 0.0f, 0.0f, s);  // SampleLevel(uv, 0): lambda = 0 + sampler bias, clamped
            }
        }
        for (int k = 0; k < 3; k++) color[k] = s[k] * mat.emission_factor[k];
    }
    float p[4];
    mat_vec4(prim.model, a.positions[3 * (size_t)i], a.positions[3 * (size_t)i + 1], a.positions[3 * (size_t)i + 2], 1.0f, p);
    sah_packed_vpl out;
    out.data[0] = pack_half2(p[0], p[1]);
    out.data[1] = pack_half2(p[2], color[0]);
    out.data[2] = pack_half2(color[1], color[2]);
    uint32_t w = 0;
    for (int k = 0; k < 3; k++) {
        const float c = __builtin_fminf(__builtin_fmaxf(v.normal[k], -1.0f), 1.0f);
        w |= ((uint32_t)((int)__builtin_rintf(c * 127.0f) & 0xff)) << (8 * k);
    }
    out.data[3] = w;  // packSnorm4x8(vec4(n, 0)): the fourth byte is 0
    a.out[i] = out;
}

// ---- injection ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kChunk = 32;              // cloud records per launch, passed by value
constexpr uint32_t kDropped = 1u << 17;      // key of an entry that is not drawn: above every cell (the volume has at most 2^17 texels)
constexpr uint32_t kTileThreads = 256, kTileRounds = 8, kTileElems = kTileThreads * kTileRounds;
constexpr uint32_t kDigitBits = 6, kDigits = 1u << kDigitBits, kPasses = 3;  // 18 key bits

struct CloudRec {
    const sah_packed_vpl* vpls;
    uint32_t count, primitive, base, padding;  // base: first point of the cloud in the per-cascade sequence
    float lo[3], hi[3];                        // mesh bounds (the model is applied on the device)
};
struct Chunk {
    CloudRec rec[kChunk];
    uint32_t num, first_base, points;  // clouds, base of the first, points of the chunk
};
struct MlArgs {
    const sah_primitive* primitives;
    const sah_material* materials;
    const sah_material_textures* material_textures;  // NULL when the scene has no texture table
    uint32_t num_primitives, num_materials;
    uint32_t num_cascades, total_points, total_entries;  // S = points per cascade, T = S * num_cascades
    float world_to_cascade[4][16];
    float min_bounds[4][3], max_bounds[4][3];
    VolumeArg rgb[3];
    uint32_t* keys;                  // T sorted keys (the general form's final buffer)
    uint32_t* vals;                  // T sequence indices in sorted order
    const sah_packed_vpl** src;      // T: where the VPL of sequence index e lives
    float* terms;                    // 12 blend sources per sorted entry, 16-byte aligned
};
struct Stage {  // what inject_one reads of one cascade
    const float* world_to_cascade;
    float cascade_f, num_cascades_f;
    const VolumeArg* rgb;
};
SAH_DEV Stage stage_of(const MlArgs& m, uint32_t c) { return Stage{m.world_to_cascade[c], (float)c, (float)m.num_cascades, m.rgb}; }

// get_primitives_in_bounds + the `emissive` test of one cloud for cascade c
SAH_DEV bool selected(const MlArgs& m, const CloudRec& r, uint32_t c) {
    if (r.primitive >= m.num_primitives) return false;
    const sah_primitive& p = m.primitives[r.primitive];
    if (p.type != SAH_PRIMITIVE_TYPE_SOLID || p.material >= m.num_materials) return false;
    const float* e = m.materials[p.material].emission_factor;
    const bool textured = m.material_textures && m.material_textures[p.material].emission != SAH_TEXTURE_NONE;
    if (!(__builtin_sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) > 0.0f) && !textured) return false;
    float lo[4], hi[4];
    mat_vec4(p.model, r.lo[0], r.lo[1], r.lo[2], 1.0f, lo);
    mat_vec4(p.model, r.hi[0], r.hi[1], r.hi[2], 1.0f, hi);
    for (int k = 0; k < 3; k++)
        if (!(m.min_bounds[c][k] < hi[k] && m.max_bounds[c][k] > lo[k])) return false;
    return true;
}
// the record holding point q of the chunk (q relative to the chunk's first point)
SAH_DEV const CloudRec& find_rec(const Chunk& ch, uint32_t q) {
    uint32_t k = 0;
    while (k + 1 < ch.num && q >= ch.rec[k + 1].base - ch.first_base) k++;
    return ch.rec[k];
}
SAH_DEV void store_terms(const Injected& v, float* rec) {
    for (int ch = 0; ch < 3; ch++)
        for (int k = 0; k < 4; k++) rec[ch * 4 + k] = v.sh[k] * v.corrected[ch] / 3.1415927f;
}
// adds the run that starts at `begin` (the entries j < n with key_at(j) == cell, contiguous) onto its texel: one rounding to half per add,
// in order.  The run is read in blocks of kRunBlock entries whose keys and terms are all loaded before the block's adds, so that a long
// run (a hot cell) waits for memory once per block rather than once per light.
constexpr int kRunBlock = 8;
template <class KeyAt> SAH_DEV void add_run(const VolumeArg* rgb, uint32_t cell, const float* terms, uint32_t begin, uint32_t n, KeyAt key_at) {
    const uint32_t W = rgb[0].width, H = rgb[0].height;
    const uint32_t cx = cell % W, cy = (cell / W) % H, cz = cell / (W * H);
    float acc[12];
    uint16_t* dst[3];
    for (int ch = 0; ch < 3; ch++) {
        dst[ch] = (uint16_t*)(rgb[ch].ptr + (size_t)cz * rgb[ch].slice_pitch + (size_t)cy * rgb[ch].row_pitch + (size_t)cx * 8);
        for (int k = 0; k < 4; k++) acc[ch * 4 + k] = h2f(dst[ch][k]);
    }
    for (uint32_t j = begin;; j += kRunBlock) {
        bool in[kRunBlock];
        float4 q[kRunBlock][3];
#pragma unroll
        for (int u = 0; u < kRunBlock; u++) in[u] = j + u < n && key_at(j + u) == cell;
#pragma unroll
        for (int u = 0; u < kRunBlock; u++)
            if (in[u]) {
                const float4* rec = reinterpret_cast<const float4*>(terms + (size_t)(j + u) * 12u);
                q[u][0] = rec[0]; q[u][1] = rec[1]; q[u][2] = rec[2];
            }
#pragma unroll
        for (int u = 0; u < kRunBlock; u++) {
            if (!in[u]) break;  // the run is contiguous: the rest of the block is past its end
            const float src[12] = {q[u][0].x, q[u][0].y, q[u][0].z, q[u][0].w, q[u][1].x, q[u][1].y, q[u][1].z, q[u][1].w,
                                   q[u][2].x, q[u][2].y, q[u][2].z, q[u][2].w};
#pragma unroll
            for (int c = 0; c < 12; c++) acc[c] = rh(acc[c] + src[c]);  // blend ONE / ONE, one rounding to half
        }
        if (!in[kRunBlock - 1]) break;
    }
    for (int ch = 0; ch < 3; ch++)
        for (int k = 0; k < 4; k++) dst[ch][k] = f2h(acc[ch * 4 + k]);
}

// Small form: every entry of the call in one workgroup (T <= kSortCapacity, one chunk).
__global__ __launch_bounds__(1024) void k_ml_small(const MlArgs m, const Chunk ch) {
    __shared__ unsigned long long s_buf[2][kSortCapacity];
    const uint32_t T = m.total_entries, S = m.total_points, t = threadIdx.x;
    unsigned long long key[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) {
        const uint32_t e = r * 1024u + t;
        uint32_t cell = ~0u;
        if (e < T) {
            const uint32_t c = e / S, q = e % S;
            const CloudRec& rec = find_rec(ch, q);
            if (selected(m, rec, c)) {
                Injected tmp;
                cell = inject_one(stage_of(m, c), rec.vpls[q - rec.base], tmp);
            }
        }
        key[r] = ((unsigned long long)cell << 32) | e;
    }
    unsigned long long* s_key = bitonic_sort_4096(key, s_buf);
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) s_key[r * 1024u + t] = key[r];
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) {
        const uint32_t i = r * 1024u + t;
        if (i < T && (uint32_t)(s_key[i] >> 32) != ~0u) {
            const uint32_t e = (uint32_t)s_key[i], c = e / S, q = e % S;
            const CloudRec& rec = find_rec(ch, q);
            Injected v;
            inject_one(stage_of(m, c), rec.vpls[q - rec.base], v);
            store_terms(v, m.terms + (size_t)i * 12u);
        }
    }
    __syncthreads();
    for (uint32_t i = t; i < T; i += 1024) {
        const uint32_t cell = (uint32_t)(s_key[i] >> 32);
        if (cell == ~0u || (i > 0 && (uint32_t)(s_key[i - 1] >> 32) == cell)) continue;
        add_run(m.rgb, cell, m.terms, i, T, [s_key](uint32_t j) { return (uint32_t)(s_key[j] >> 32); });
    }
}

// General form, step 1: the entries of one chunk of clouds, for every cascade.
__global__ __launch_bounds__(256) void k_ml_eval(const MlArgs m, const Chunk ch, uint32_t* keys) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ch.points * m.num_cascades) return;
    const uint32_t c = i / ch.points, q = i % ch.points;
    const CloudRec& rec = find_rec(ch, q);
    const uint32_t p = q - (rec.base - ch.first_base);
    const uint32_t e = c * m.total_points + rec.base + p;
    uint32_t cell = kDropped;
    if (selected(m, rec, c)) {
        Injected tmp;
        const uint32_t got = inject_one(stage_of(m, c), rec.vpls[p], tmp);
        if (got != ~0u) cell = got;
    }
    keys[e] = cell;
    m.src[e] = rec.vpls + p;
}

// Step 2: LSD radix sort.  Tiles of kTileElems consecutive entries; digit counts per tile, [digit][tile] order.
__global__ __launch_bounds__(kTileThreads) void k_rs_hist(const uint32_t* keys, uint32_t n, uint32_t shift, uint32_t* hist, uint32_t num_tiles) {
    __shared__ uint32_t s_h[kDigits];
    const uint32_t t = threadIdx.x, tile = blockIdx.x;
    if (t < kDigits) s_h[t] = 0;
    __syncthreads();
    for (uint32_t r = 0; r < kTileRounds; r++) {
        const uint32_t idx = tile * kTileElems + r * kTileThreads + t;
        if (idx < n) atomicAdd(&s_h[(keys[idx] >> shift) & (kDigits - 1)], 1u);
    }
    __syncthreads();
    if (t < kDigits) hist[t * num_tiles + tile] = s_h[t];
}
// exclusive scan of len counts, one workgroup: a contiguous slice per thread, a scan of the slice sums in LDS
__global__ __launch_bounds__(1024) void k_rs_scan(uint32_t* hist, uint32_t len) {
    __shared__ uint32_t s_sum[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (len + 1023) / 1024, begin = min(t * per, len), end = min(begin + per, len);
    uint32_t sum = 0;
    for (uint32_t i = begin; i < end; i++) sum += hist[i];
    s_sum[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint32_t add = t >= d ? s_sum[t - d] : 0u;
        __syncthreads();
        s_sum[t] += add;
        __syncthreads();
    }
    uint32_t run = s_sum[t] - sum;
    for (uint32_t i = begin; i < end; i++) {
        const uint32_t c = hist[i];
        hist[i] = run;
        run += c;
    }
}
// stable scatter: within a tile entries are ranked in index order (round by round; inside a round by wave, then lane)
__global__ __launch_bounds__(kTileThreads) void k_rs_scatter(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out,
                                                            uint32_t n, uint32_t shift, const uint32_t* hist, uint32_t num_tiles) {
    constexpr uint32_t kWaves = kTileThreads / 64;
    __shared__ uint32_t s_run[kDigits];
    __shared__ uint32_t s_wave[kWaves][kDigits];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, tile = blockIdx.x;
    if (t < kDigits) s_run[t] = hist[t * num_tiles + tile];
    for (uint32_t r = 0; r < kTileRounds; r++) {
        const uint32_t idx = tile * kTileElems + r * kTileThreads + t;
        const bool valid = idx < n;
        const uint32_t key = valid ? keys_in[idx] : 0u;
        const uint32_t d = (key >> shift) & (kDigits - 1);
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < kDigitBits; b++) {
            const uint64_t set = __ballot(((d >> b) & 1u) != 0u);
            peers &= ((d >> b) & 1u) ? set : ~set;
        }
        s_wave[wave][lane] = 0;
        __syncthreads();
        const uint32_t rank = (uint32_t)__builtin_popcountll(peers & ((1ull << lane) - 1ull));
        if (valid && (peers >> lane) == 1ull) s_wave[wave][d] = (uint32_t)__builtin_popcountll(peers);  // the last lane of its digit
        __syncthreads();
        if (valid) {
            uint32_t pos = s_run[d] + rank;
            for (uint32_t w = 0; w < wave; w++) pos += s_wave[w][d];
            keys_out[pos] = key;
            vals_out[pos] = vals_in ? vals_in[idx] : idx;
        }
        __syncthreads();
        if (t < kDigits) {
            uint32_t add = 0;
            for (uint32_t w = 0; w < kWaves; w++) add += s_wave[w][t];
            s_run[t] += add;
        }
        __syncthreads();
    }
}

// Step 3: the blend sources in sorted order.
__global__ __launch_bounds__(256) void k_ml_terms(const MlArgs m) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m.total_entries || m.keys[i] == kDropped) return;
    const uint32_t e = m.vals[i], c = e / m.total_points;
    Injected v;
    inject_one(stage_of(m, c), *m.src[e], v);
    store_terms(v, m.terms + (size_t)i * 12u);
}
// Step 4: one walker per run.
__global__ __launch_bounds__(256) void k_ml_walk(const MlArgs m) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t T = m.total_entries;
    if (i >= T) return;
    const uint32_t cell = m.keys[i];
    if (cell == kDropped || (i > 0 && m.keys[i - 1] == cell)) return;
    const uint32_t* keys = m.keys;
    add_run(m.rgb, cell, m.terms, i, T, [keys](uint32_t j) { return keys[j]; });
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

hipError_t launch_emissive_vpls(const EmissiveArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_emissive_vpls, dim3((a.num_points + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

// bytes of scratch the general form needs for T entries
size_t ml_scratch_bytes(uint32_t T) {
    const size_t tiles = (T + kTileElems - 1) / kTileElems;
    return 4 * align256((size_t)T * 4) + align256((size_t)T * sizeof(void*)) + align256((size_t)T * 48) + align256(tiles * kDigits * 4);
}

// clouds: the records with count > 0, bases filled in; S = their total count
hipError_t launch_inject_emissive(MlArgs m, const std::vector<CloudRec>& clouds, void* scratch, hipStream_t st) {
    const uint32_t T = m.total_entries, S = m.total_points;
    uint8_t* p = (uint8_t*)scratch;
    auto take = [&p](size_t bytes) { uint8_t* q = p; p += align256(bytes); return q; };
    if (T <= kSortCapacity && clouds.size() <= kChunk) {
        Chunk ch{};
        for (size_t k = 0; k < clouds.size(); k++) ch.rec[k] = clouds[k];
        ch.num = (uint32_t)clouds.size();
        ch.first_base = 0;
        ch.points = S;
        m.terms = (float*)take((size_t)kSortCapacity * 48);
        hipLaunchKernelGGL(k_ml_small, dim3(1), dim3(1024), 0, st, m, ch);
        return hipGetLastError();
    }
    const uint32_t tiles = (T + kTileElems - 1) / kTileElems;
    uint32_t* keys[2] = {(uint32_t*)take((size_t)T * 4), (uint32_t*)take((size_t)T * 4)};
    uint32_t* vals[2] = {(uint32_t*)take((size_t)T * 4), (uint32_t*)take((size_t)T * 4)};
    m.src = (const sah_packed_vpl**)take((size_t)T * sizeof(void*));
    m.terms = (float*)take((size_t)T * 48);
    uint32_t* hist = (uint32_t*)take((size_t)tiles * kDigits * 4);
    for (size_t k0 = 0; k0 < clouds.size(); k0 += kChunk) {
        Chunk ch{};
        ch.num = (uint32_t)std::min<size_t>(kChunk, clouds.size() - k0);
        for (uint32_t k = 0; k < ch.num; k++) ch.rec[k] = clouds[k0 + k];
        ch.first_base = ch.rec[0].base;
        ch.points = ch.rec[ch.num - 1].base + ch.rec[ch.num - 1].count - ch.first_base;
        const uint32_t n = ch.points * m.num_cascades;
        hipLaunchKernelGGL(k_ml_eval, dim3((n + 255) / 256), dim3(256), 0, st, m, ch, keys[0]);
    }
    for (uint32_t pass = 0; pass < kPasses; pass++) {
        const uint32_t shift = pass * kDigitBits, in = pass & 1u;
        hipLaunchKernelGGL(k_rs_hist, dim3(tiles), dim3(kTileThreads), 0, st, keys[in], T, shift, hist, tiles);
        hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, st, hist, tiles * kDigits);
        hipLaunchKernelGGL(k_rs_scatter, dim3(tiles), dim3(kTileThreads), 0, st, keys[in], pass == 0 ? (const uint32_t*)nullptr : vals[in], keys[in ^ 1u],
                           vals[in ^ 1u], T, shift, hist, tiles);
    }
    m.keys = keys[kPasses & 1u];
    m.vals = vals[kPasses & 1u];
    const dim3 grid((T + 255) / 256);
    hipLaunchKernelGGL(k_ml_terms, grid, dim3(256), 0, st, m);
    hipLaunchKernelGGL(k_ml_walk, grid, dim3(256), 0, st, m);
    return hipGetLastError();
}

}  // namespace sah

// ---- host: the point cloud of a mesh (mesh_storage.cpp:246-450, with the choices sah_lpv_mesh_lights.h pins) ------------------------------
namespace {
struct MinStd0 {  // minstd_rand0
    uint64_t x;
    explicit MinStd0(uint64_t seed) {
        x = seed % 2147483647u;
        if (x == 0) x = 1;
    }
    uint32_t next() {
        x = (x * 16807u) % 2147483647u;
        return (uint32_t)x;
    }
};
// libstdc++'s generate_canonical<double, 53> over minstd_rand0 (two draws), as uniform_real_distribution<double>{0, 1} returns it
double uniform01(MinStd0& e) {
    const double R = 2147483646.0;
    double sum = 0.0, tmp = 1.0;
    for (int k = 0; k < 2; k++) {
        sum += (double)(e.next() - 1u) * tmp;
        tmp *= R;
    }
    double ret = sum / tmp;
    if (ret >= 1.0) ret = std::nextafter(1.0, 0.0);
    return ret;
}
float length3(const float v[3]) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
uint32_t pack_unorm4x8(const float c[4]) {
    uint32_t out = 0;
    for (int k = 0; k < 4; k++) {
        float v = c[k];
        v = (v < 0.0f) ? 0.0f : v;  // glm::clamp = min(max(v, 0), 1) with max(x, y) = x < y ? y : x, min(x, y) = y < x ? y : x
        v = (1.0f < v) ? 1.0f : v;
        const float r = std::round(v * 255.0f);
        out |= (r == r ? (uint32_t)r : 0u) << (8 * k);
    }
    return out;
}
}  // namespace

extern "C" {

int sah_mesh_point_cloud(const float* positions, const sah_vertex_data* vertex_data, uint32_t num_vertices, const uint32_t* indices,
                         uint32_t num_indices, uint32_t first_index, uint32_t index_count, int32_t vertex_offset, uint64_t seed, uint32_t flags,
                         float* out_positions, sah_vertex_data* out_points, uint32_t capacity, uint32_t* out_count, float bounds_min[3],
                         float bounds_max[3]) {
    if (!out_count || (flags & ~SAH_POINT_CLOUD_ON_SURFACE) || index_count % 3 != 0 || (uint64_t)first_index + index_count > num_indices) return SAH_ERR_INVALID_ARGUMENT;
    if (index_count && (!positions || !vertex_data || !indices)) return SAH_ERR_INVALID_ARGUMENT;
    if ((out_positions == nullptr) != (out_points == nullptr) || (!out_positions && capacity)) return SAH_ERR_INVALID_ARGUMENT;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < index_count; i++) {
        const int64_t v = (int64_t)indices[first_index + i] + vertex_offset;
        if (v < 0 || v >= (int64_t)num_vertices) return SAH_ERR_INVALID_ARGUMENT;
        for (int k = 0; k < 3; k++) {
            lo[k] = std::fmin(lo[k], positions[3 * v + k]);
            hi[k] = std::fmax(hi[k], positions[3 * v + k]);
        }
    }
    if (bounds_min) std::memcpy(bounds_min, lo, sizeof lo);
    if (bounds_max) std::memcpy(bounds_max, hi, sizeof hi);
    const uint32_t num_tris = index_count / 3;
    auto vtx = [&](uint32_t tri, int corner) { return (uint32_t)((int64_t)indices[first_index + 3 * tri + corner] + vertex_offset); };
    std::vector<double> prefix(num_tris);
    double total = 0.0;
    for (uint32_t t = 0; t < num_tris; t++) {
        const float* p0 = positions + 3 * (size_t)vtx(t, 0);
        const float* p1 = positions + 3 * (size_t)vtx(t, 1);
        const float* p2 = positions + 3 * (size_t)vtx(t, 2);
        const float a[3] = {p0[0] - p1[0], p0[1] - p1[1], p0[2] - p1[2]}, b[3] = {p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2]};
        const float c[3] = {a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]};
        prefix[t] = (double)length3(c) / 2.0;
        total += prefix[t];
    }
    uint32_t count = 0;
    if (std::isfinite(total) && total > 0.0) count = (uint32_t)std::min(std::ceil(total / 0.1), 65536.0);
    *out_count = count;
    if (!out_positions) return SAH_OK;
    if (capacity < count) return SAH_ERR_INVALID_ARGUMENT;
    double run = 0.0;
    for (uint32_t t = 0; t < num_tris; t++) {
        run += prefix[t] / total;
        prefix[t] = run;
    }
    const bool on_surface = (flags & SAH_POINT_CLOUD_ON_SURFACE) != 0;
    MinStd0 engine(seed);
    for (uint32_t i = 0; i < count; i++) {
        const double u = uniform01(engine);
        uint32_t tri = (uint32_t)(std::upper_bound(prefix.begin(), prefix.end(), u) - prefix.begin());
        if (tri == num_tris) tri = num_tris - 1;
        float bc[3];
        for (int k = 0; k < 3; k++) bc[k] = (float)uniform01(engine);
        const float inv = 1.0f / length3(bc);
        float w[3] = {bc[0] * inv, bc[1] * inv, bc[2] * inv};
        if (on_surface) {
            const float s = (w[0] + w[1]) + w[2];
            for (int k = 0; k < 3; k++) w[k] = w[k] / s;
        }
        const float div = on_surface ? 1.0f : 3.0f;
        const uint32_t v[3] = {vtx(tri, 0), vtx(tri, 1), vtx(tri, 2)};
        auto mix = [&](float a0, float a1, float a2) {
            const float s = (a0 * w[0] + a1 * w[1]) + a2 * w[2];
            return on_surface ? s : s / div;
        };
        for (int k = 0; k < 3; k++) out_positions[3 * (size_t)i + k] = mix(positions[3 * (size_t)v[0] + k], positions[3 * (size_t)v[1] + k], positions[3 * (size_t)v[2] + k]);
        sah_vertex_data& o = out_points[i];
        const sah_vertex_data &d0 = vertex_data[v[0]], &d1 = vertex_data[v[1]], &d2 = vertex_data[v[2]];
        for (int k = 0; k < 3; k++) o.normal[k] = mix(d0.normal[k], d1.normal[k], d2.normal[k]);
        for (int k = 0; k < 4; k++) o.tangent[k] = mix(d0.tangent[k], d1.tangent[k], d2.tangent[k]);
        for (int k = 0; k < 2; k++) o.texcoord[k] = mix(d0.texcoord[k], d1.texcoord[k], d2.texcoord[k]);
        float col[4];
        for (int k = 0; k < 4; k++) {
            const float s = 0.0039215686274509803921568627451f;  // glm::unpackUnorm4x8
            col[k] = mix((float)((d0.color >> (8 * k)) & 0xffu) * s, (float)((d1.color >> (8 * k)) & 0xffu) * s, (float)((d2.color >> (8 * k)) & 0xffu) * s);
        }
        o.color = pack_unorm4x8(col);
    }
    return SAH_OK;
}

int sah_lpv_emissive_vpls(sah_ctx* ctx, const sah_scene_geometry* scene, uint32_t primitive_index, const float* positions,
                          const sah_vertex_data* points, uint32_t num_points, uint32_t flags, sah_packed_vpl* out_vpls) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!scene || !scene->primitives || !scene->materials || primitive_index >= scene->num_primitives || (flags & ~SAH_EMISSIVE_MATERIAL_ZERO))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lpv_emissive_vpls: null scene arrays, primitive index beyond the scene or unknown flags");
    if (num_points && (!positions || !points || !out_vpls)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lpv_emissive_vpls: null point or VPL array");
    if (num_points == 0) return SAH_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    sah::EmissiveArgs a{};
    a.luts = ctx->luts;
    a.primitives = scene->primitives;
    a.materials = scene->materials;
    const bool textured = scene->textures && scene->material_textures && scene->num_textures;
    a.material_textures = textured ? scene->material_textures : nullptr;
    a.textures = textured ? scene->textures : nullptr;
    a.num_textures = textured ? scene->num_textures : 0;
    a.num_materials = scene->num_materials;
    a.primitive = primitive_index;
    a.flags = flags;
    a.num_points = num_points;
    a.positions = positions;
    a.points = points;
    a.out = out_vpls;
    HIP_TRY(ctx, sah::launch_emissive_vpls(a, ctx->stream));
    return SAH_OK;
}

int sah_lpv_inject_emissive(sah_ctx* ctx, const sah_scene_geometry* scene, const sah_emissive_cloud* clouds, uint32_t num_clouds,
                            const sah_lpv_cascade_matrices* cascades, const sah_lpv_cascade_bounds* bounds, uint32_t num_cascades,
                            const sah_volume a_rgb[3]) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!scene || (num_clouds && !clouds) || !cascades || !bounds || !a_rgb || num_cascades == 0 || num_cascades > 4)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lpv_inject_emissive: null argument or cascade count outside [1, 4]");
    const sah_volume& v0 = a_rgb[0];
    for (int c = 0; c < 3; c++) {
        const sah_volume& v = a_rgb[c];
        if (!v.ptr || v.format != SAH_FORMAT_R16G16B16A16_SFLOAT || v.width != v0.width || v.height != v0.height || v.depth != v0.depth || !v.width ||
            !v.height || !v.depth || (uint64_t)v.width * v.height * v.depth > (1ull << 17) || (uint64_t)v.row_pitch_bytes < (uint64_t)v.width * 8 ||
            (uint64_t)v.slice_pitch_bytes < (uint64_t)v.row_pitch_bytes * v.height || ((uintptr_t)v.ptr % 8) || (v.row_pitch_bytes % 8) ||
            (v.slice_pitch_bytes % 8))
            return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "lpv_inject_emissive: three RGBA16F volumes of one extent with at most 2^17 texels, 8-byte aligned");
    }
    std::vector<sah::CloudRec> recs;
    uint64_t S = 0;
    for (uint32_t k = 0; k < num_clouds; k++) {
        const sah_emissive_cloud& c = clouds[k];
        if (c.count == 0) continue;
        if (!c.vpls) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lpv_inject_emissive: cloud %u has points but no VPL list", k);
        sah::CloudRec r{};
        r.vpls = c.vpls;
        r.count = c.count;
        r.primitive = c.primitive;
        r.base = (uint32_t)std::min<uint64_t>(S, 0xffffffffu);
        for (int i = 0; i < 3; i++) { r.lo[i] = c.bounds_min[i]; r.hi[i] = c.bounds_max[i]; }
        recs.push_back(r);
        S += c.count;
    }
    const uint64_t T = S * num_cascades;
    if (T > SAH_LPV_EMISSIVE_MAX_ENTRIES)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lpv_inject_emissive: %llu entries (points x cascades), more than %u", (unsigned long long)T,
                    SAH_LPV_EMISSIVE_MAX_ENTRIES);
    if (T == 0) return SAH_OK;
    if (!scene->primitives || !scene->materials) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "lpv_inject_emissive: the scene needs primitives and materials");
    ctx->lpv_copy.drop(ctx->cache_epoch);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    sah::MlArgs m{};
    m.primitives = scene->primitives;
    m.materials = scene->materials;
    const bool textured = scene->textures && scene->material_textures && scene->num_textures;
    m.material_textures = textured ? scene->material_textures : nullptr;
    m.num_primitives = scene->num_primitives;
    m.num_materials = scene->num_materials;
    m.num_cascades = num_cascades;
    m.total_points = (uint32_t)S;
    m.total_entries = (uint32_t)T;
    for (uint32_t c = 0; c < num_cascades; c++) {
        std::memcpy(m.world_to_cascade[c], cascades[c].world_to_cascade, 64);
        std::memcpy(m.min_bounds[c], bounds[c].min_bounds, 12);
        std::memcpy(m.max_bounds[c], bounds[c].max_bounds, 12);
    }
    for (int c = 0; c < 3; c++) m.rgb[c] = varg(a_rgb[c]);
    // scratch grows only; freeing a smaller one waits for the work that may still use it
    const size_t need = sah::ml_scratch_bytes((uint32_t)std::max<uint64_t>(T, 4096));
    HIP_TRY(ctx, ctx->ml_scratch.grow(ctx->stream, need));
    HIP_TRY(ctx, sah::launch_inject_emissive(m, recs, ctx->ml_scratch.ptr, ctx->stream));
    return SAH_OK;
}

}  // extern "C"
