// The LPV geometry volume (GV) producers (include/sah_lpv_gv.h):
//   "Inject RSM depth into GV"    RenderCore/shaders/gi/lpv/gv_injection.{vert,frag}                (host light_propagation_volume.cpp:1065-1128)
//   "Inject scene depth into GV"  RenderCore/shaders/gi/lpv/inject_scene_depth_into_gv.{vert,geom,frag} (host :932-968)
// Both are point lists with MAX blending into the RGBA16F GV.  MAX is order-independent, so the scatter is deterministic without ordering:
// every point's half4 is turned into four order-preserving 16-bit keys (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN),
// a workgroup reduces its points per cell in an LDS hash table (ds_max_u32), and each distinct cell-channel of a workgroup issues one global
// atomic max into a 32-bit key scratch that k_gv_seed filled from the GV and k_gv_resolve writes back.  Arithmetic: GLSL fp32, every operator
// rounded (the shaders' mediump is evaluated in fp32).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sah_hip.h"
#include "launch.hpp"
#include "numerics.hpp"
#include "params.hpp"

namespace sah {
namespace {

constexpr uint32_t kGvThreads = 256, kGvPerThread = 4, kGvPointsPerBlock = kGvThreads * kGvPerThread;
constexpr uint32_t kGvSlots = 2048;  // >= 2 x the points of a workgroup: the linear probe always finds a slot
constexpr uint32_t kEmpty = 0xffffffffu;

// order-preserving key of a half's bit pattern; 0 (the key of 0xffff, a NaN) doubles as "no value" in LDS: sources are never NaN
SAH_DEV uint32_t gv_key(uint32_t h) { return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u); }
SAH_DEV uint32_t gv_unkey(uint32_t k) { return (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu); }

SAH_DEV void mat_vec4(const float* m, float x, float y, float z, float w, float out[4]) {
    for (int r = 0; r < 4; r++) out[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w;
}

struct GvInjectArgs {
    VolumeArg gv;
    uint32_t* keys;  // 4 per GV texel, x + W (y + H z)
    float W, H, D, num_cascades_f;
    uint32_t first_cascade;
    uint32_t num_vertices;
    // RSM: normals (R8G8B8A8_UNORM) and depth (D16_UNORM) arrays, one layer per cascade
    VolumeArg rsm_normals, rsm_depth;
    uint32_t res_x, res_y;
    float inverse_rsm_vp[4][16];
    // scene: depth (D32_SFLOAT) and normals (R16G16B16A16_SFLOAT) planes
    PlaneArg depth, normals;
    uint32_t width, height;
    float inverse_view[16], inverse_projection[16];
    float world_to_cascade[4][16];
};

struct GvPoint {
    uint32_t cell;  // kEmpty: dropped
    uint32_t key[4];
};

// dir_to_cosine_lobe(normal) (spherical_harmonics.glsl:28-30) in fp32, stored as half: the blend source
SAH_DEV void lobe_keys(const float n[3], uint32_t key[4]) {
    const float c0 = 0.886226925f, c1 = 1.02332671f;
    const float v[4] = {c0, -c1 * n[1], c1 * n[2], -c1 * n[0]};
    for (int k = 0; k < 4; k++) key[k] = isnan_f(v[k]) ? 0u : gv_key(f2h(v[k]));  // a NaN source leaves its channel as it was
}
// gl_Position (ndc_x, ndc_y, 0, 1) and gl_Layer = int(layer_f) -> the texel: the rule of sah_lpv_inject_vpls (vpl.hip: inject_one)
SAH_DEV uint32_t point_cell(const GvInjectArgs& a, float ndc_x, float ndc_y, float layer_f) {
    const float xf = ndc_x * (a.W * 0.5f) + a.W * 0.5f, yf = ndc_y * (a.H * 0.5f) + a.H * 0.5f;
    if (!(xf >= 0.0f && xf < a.W && yf >= 0.0f && yf < a.H)) return kEmpty;
    if (!(layer_f > -1.0f && layer_f < a.D)) return kEmpty;
    const uint32_t cx = (uint32_t)__builtin_floorf(xf), cy = (uint32_t)__builtin_floorf(yf), cz = (uint32_t)(int)layer_f;
    return cx + a.gv.width * (cy + a.gv.height * cz);
}
SAH_DEV bool outside01(const float c[4]) { return c[0] < 0.0f || c[1] < 0.0f || c[2] < 0.0f || c[0] > 1.0f || c[1] > 1.0f || c[2] > 1.0f; }

// gv_injection.vert, vertex i of cascade c
SAH_DEV GvPoint rsm_point(const GvInjectArgs& a, uint32_t c, uint32_t i) {
    GvPoint p;
    p.cell = kEmpty;
    const uint64_t t = 2ull * i;
    const uint32_t x = (uint32_t)(t % a.res_x);
    const uint64_t y64 = t / a.res_x;
    if (y64 >= a.res_y) return p;
    const uint32_t y = (uint32_t)y64;
    const float rx = (float)a.res_x, ry = (float)a.res_y;
    const float tu = (0.5f + (float)x) / rx, tv = (0.5f + (float)y) / ry;
    // the default sampler: NEAREST, REPEAT (texel floor(u * res) wrapped), layer c
    int ix = (int)__builtin_floorf(tu * rx) % (int)a.res_x, iy = (int)__builtin_floorf(tv * ry) % (int)a.res_y;
    if (ix < 0) ix += (int)a.res_x;
    if (iy < 0) iy += (int)a.res_y;
    const uint8_t* dp = a.rsm_depth.ptr + (size_t)c * a.rsm_depth.slice_pitch + (size_t)iy * a.rsm_depth.row_pitch + (size_t)ix * 2;
    const uint8_t* np = a.rsm_normals.ptr + (size_t)c * a.rsm_normals.slice_pitch + (size_t)iy * a.rsm_normals.row_pitch + (size_t)ix * 4;
    const float depth = (float)*(const uint16_t*)dp / 65535.0f;
    const float ndc[2] = {((float)x / rx) * 2.0f - 1.0f, ((float)y / ry) * 2.0f - 1.0f};
    const float identity[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float vs[4], ws[4], cp[4];
    mat_vec4(identity, ndc[0], ndc[1], depth, 1.0f, vs);  // inverse_projection = I (:1080-1084)
    const float w = vs[3];
    for (int k = 0; k < 4; k++) vs[k] = vs[k] / w;
    mat_vec4(a.inverse_rsm_vp[c], vs[0], vs[1], vs[2], vs[3], ws);
    mat_vec4(a.world_to_cascade[c], ws[0], ws[1], ws[2], ws[3], cp);
    if (outside01(cp)) return p;
    const float n[3] = {(float)np[0] / 255.0f, (float)np[1] / 255.0f, (float)np[2] / 255.0f};  // UNORM as read: no * 2 - 1
    lobe_keys(n, p.key);
    for (int k = 0; k < 4; k++) cp[k] = cp[k] + 0.5f / 32.f;
    const float px = (cp[0] + (float)c) / a.num_cascades_f;
    p.cell = point_cell(a, px * 2.0f - 1.0f, cp[1] * 2.0f - 1.0f, cp[2] * 32.0f);
    return p;
}

// inject_scene_depth_into_gv.vert (vertex i) + .geom (the primitive it emits for cascade c)
SAH_DEV GvPoint scene_point(const GvInjectArgs& a, uint32_t c, uint32_t i) {
    GvPoint p;
    p.cell = kEmpty;
    const uint32_t x = i % a.width, y = i / a.width;
    const float depth = *(const float*)(a.depth.ptr + (size_t)y * a.depth.pitch + (size_t)x * 4);
    const float ss[2] = {((float)x + 0.5f) / (float)a.width, ((float)y + 0.5f) / (float)a.height};
    float vs[4], ws[4], cp[4];
    mat_vec4(a.inverse_projection, ss[0] * 2.0f - 1.0f, ss[1] * 2.0f - 1.0f, depth, 1.0f, vs);
    const float w = vs[3];
    for (int k = 0; k < 4; k++) vs[k] = vs[k] / w;
    mat_vec4(a.inverse_view, vs[0], vs[1], vs[2], vs[3], ws);
    mat_vec4(a.world_to_cascade[c], ws[0], ws[1], ws[2], ws[3], cp);
    if (outside01(cp)) return p;  // gl_Position = vec4(-1): clipped
    const uint16_t* nh = (const uint16_t*)(a.normals.ptr + (size_t)y * a.normals.pitch + (size_t)x * 8);
    const float n[3] = {h2f(nh[0]), h2f(nh[1]), h2f(nh[2])};  // texelFetch, not normalised
    lobe_keys(n, p.key);
    p.cell = point_cell(a, (cp[0] + (float)c) / a.num_cascades_f, cp[1], cp[2] * 32.0f);  // no * 2 - 1, no half-cell offset
    return p;
}

__global__ __launch_bounds__(256) void k_gv_seed(const VolumeArg gv, uint32_t* keys) {
    const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= gv.width * gv.height * gv.depth) return;
    const uint32_t x = cell % gv.width, y = (cell / gv.width) % gv.height, z = cell / (gv.width * gv.height);
    const uint2 q = *reinterpret_cast<const uint2*>(gv.ptr + (size_t)z * gv.slice_pitch + (size_t)y * gv.row_pitch + (size_t)x * 8);
    *reinterpret_cast<uint4*>(keys + 4ull * cell) = make_uint4(gv_key(q.x & 0xffffu), gv_key(q.x >> 16), gv_key(q.y & 0xffffu), gv_key(q.y >> 16));
}
__global__ __launch_bounds__(256) void k_gv_resolve(const VolumeArg gv, const uint32_t* keys) {
    const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= gv.width * gv.height * gv.depth) return;
    const uint32_t x = cell % gv.width, y = (cell / gv.width) % gv.height, z = cell / (gv.width * gv.height);
    const uint4 k = *reinterpret_cast<const uint4*>(keys + 4ull * cell);
    *reinterpret_cast<uint2*>(const_cast<uint8_t*>(gv.ptr) + (size_t)z * gv.slice_pitch + (size_t)y * gv.row_pitch + (size_t)x * 8) =
        make_uint2(gv_unkey(k.x) | (gv_unkey(k.y) << 16), gv_unkey(k.z) | (gv_unkey(k.w) << 16));
}

// blockIdx.y: cascade first_cascade + y; blockIdx.x: kGvPointsPerBlock consecutive vertices
template <bool SCENE>
__global__ __launch_bounds__(256) void k_gv_inject(const GvInjectArgs a) {
    __shared__ uint32_t s_tag[kGvSlots];
    __shared__ uint32_t s_val[kGvSlots][4];
    const uint32_t t = threadIdx.x;
    for (uint32_t s = t; s < kGvSlots; s += kGvThreads) {
        s_tag[s] = kEmpty;
        s_val[s][0] = s_val[s][1] = s_val[s][2] = s_val[s][3] = 0u;
    }
    __syncthreads();
    const uint32_t c = a.first_cascade + blockIdx.y;
    for (uint32_t r = 0; r < kGvPerThread; r++) {
        const uint64_t i = (uint64_t)blockIdx.x * kGvPointsPerBlock + r * kGvThreads + t;
        if (i >= a.num_vertices) break;
        const GvPoint p = SCENE ? scene_point(a, c, (uint32_t)i) : rsm_point(a, c, (uint32_t)i);
        if (p.cell == kEmpty) continue;
        uint32_t h = (p.cell * 2654435761u) >> 21;  // 11 bits: kGvSlots
        for (;;) {  // at most kGvPointsPerBlock distinct tags in kGvSlots slots: terminates
            const uint32_t old = atomicCAS(&s_tag[h], kEmpty, p.cell);
            if (old == kEmpty || old == p.cell) break;
            h = (h + 1u) & (kGvSlots - 1u);
        }
        for (int k = 0; k < 4; k++)
            if (p.key[k] != 0u) atomicMax(&s_val[h][k], p.key[k]);
    }
    __syncthreads();
    for (uint32_t s = t; s < kGvSlots; s += kGvThreads) {
        const uint32_t cell = s_tag[s];
        if (cell == kEmpty) continue;
        for (int k = 0; k < 4; k++) {
            const uint32_t v = s_val[s][k];
            if (v != 0u) atomicMax(&a.keys[4ull * cell + k], v);
        }
    }
}

hipError_t launch_gv(GvInjectArgs& a, uint32_t cascade_count, bool scene, hipStream_t st) {
    const uint32_t cells = a.gv.width * a.gv.height * a.gv.depth;
    a.W = (float)a.gv.width;
    a.H = (float)a.gv.height;
    a.D = (float)a.gv.depth;
    hipLaunchKernelGGL(k_gv_seed, dim3((cells + 255u) / 256u), dim3(256), 0, st, a.gv, a.keys);
    if (a.num_vertices > 0 && cascade_count > 0) {
        const dim3 grid((a.num_vertices + kGvPointsPerBlock - 1u) / kGvPointsPerBlock, cascade_count);
        if (scene) hipLaunchKernelGGL(k_gv_inject<true>, grid, dim3(kGvThreads), 0, st, a);
        else hipLaunchKernelGGL(k_gv_inject<false>, grid, dim3(kGvThreads), 0, st, a);
    }
    hipLaunchKernelGGL(k_gv_resolve, dim3((cells + 255u) / 256u), dim3(256), 0, st, a.gv, (const uint32_t*)a.keys);
    return hipGetLastError();
}

}  // namespace

// rsm: normals + depth arrays (res_x x res_y, layers >= first_cascade + cascade_count); keys: 16 bytes per GV texel
hipError_t launch_gv_inject_rsm(const VolumeArg& normals, const VolumeArg& depth, const sah_lpv_cascade_matrices* cascades, uint32_t first_cascade,
                                uint32_t cascade_count, uint32_t num_cascades, const VolumeArg& gv, uint32_t* keys, hipStream_t st) {
    GvInjectArgs a{};
    a.gv = gv;
    a.keys = keys;
    a.num_cascades_f = (float)num_cascades;
    a.first_cascade = first_cascade;
    a.rsm_normals = normals;
    a.rsm_depth = depth;
    a.res_x = depth.width;
    a.res_y = depth.height;
    a.num_vertices = depth.width * depth.height;  // (host-checked: < 2^31)
    for (uint32_t c = 0; c < num_cascades; c++)
        for (int k = 0; k < 16; k++) {
            a.inverse_rsm_vp[c][k] = cascades[c].inverse_rsm_vp[k];
            a.world_to_cascade[c][k] = cascades[c].world_to_cascade[k];
        }
    return launch_gv(a, cascade_count, false, st);
}

hipError_t launch_gv_inject_scene(const PlaneArg& depth, const PlaneArg& normals, uint32_t width, uint32_t height, const sah_view_data& view,
                                  const sah_lpv_cascade_matrices* cascades, uint32_t num_cascades, const VolumeArg& gv, uint32_t* keys, hipStream_t st) {
    GvInjectArgs a{};
    a.gv = gv;
    a.keys = keys;
    a.num_cascades_f = (float)num_cascades;
    a.first_cascade = 0;
    a.depth = depth;
    a.normals = normals;
    a.width = width;
    a.height = height;
    a.num_vertices = width * height / 4u;  // draw(effective_resolution.x * effective_resolution.y / 4), uint32 (host-checked: no overflow)
    for (int k = 0; k < 16; k++) {
        a.inverse_view[k] = view.inverse_view[k];
        a.inverse_projection[k] = view.inverse_projection[k];
    }
    for (uint32_t c = 0; c < num_cascades; c++)
        for (int k = 0; k < 16; k++) a.world_to_cascade[c][k] = cascades[c].world_to_cascade[k];
    return launch_gv(a, num_cascades, true, st);
}

}  // namespace sah
