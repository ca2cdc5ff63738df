// Fused "Lighting" pass for gfx950 (MI355X): one pass over the G-buffer replaces the reference's clear + sun + GI overlay
// + emissive + sky draws and the RT-mode sun dispatch (RenderCore/render/phase/lighting_phase.cpp:99-134), reading each
// plane once and writing lit_scene once, while reproducing the intermediate RGBA16F blend roundings (DESIGN.md "a0").
//
// Three kernels:
//   k_lighting_fast     the hot kernel.  One thread shades PPT horizontally adjacent pixels (PPT=4: 16 B/lane plane loads,
//                       16 B/lane lit stores).  It exploits what the host verified about the uniform blocks (projection
//                       inverse separable in x/y/depth, affine view inverse, scale+translate LPV cascades, affine shadow
//                       matrices) and skips sub-expressions that are provably inert for the pixel at hand (DESIGN.md "Fast
//                       path proofs").  Pixels it cannot prove anything about (sky, non-finite inputs, roughness 0 under
//                       LPV GI, ...) are appended to a per-frame list with one wave-aggregated atomic.
//   k_lighting_fixup    shades the listed pixels with the general restatement (lighting_common.hpp).
//   k_lighting_general  the general restatement over the whole image: used when the uniform blocks do not have the
//                       structure the fast kernel needs, and as the in-library cross-check of the fast path.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/sah_hip.h"
#include "fast_pixel_map.hpp"
#include "lighting_common.hpp"
#include "lighting_fast.hpp"
#include "launch.hpp"
#include "numerics.hpp"
#include "params.hpp"

namespace sah {

// ---- general kernel -------------------------------------------------------------------------------------------
template <int SUN, int GI, int PPT>
__global__ void __launch_bounds__(256) k_lighting_general(const LightingArgs a, const CsmArgs csm, const LpvArgs lpv, const SkyArgs sky) {
    __shared__ float s_lut[512];
    stage_format_tables(s_lut, a.luts);
    __syncthreads();

    const uint32_t groups_per_row = a.width / PPT;
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t rows = a.row_end - a.row_begin;
    if (gid >= groups_per_row * rows) return;
    const uint32_t ry = gid / groups_per_row;
    const uint32_t y = a.row_begin + ry;
    const uint32_t x0 = (gid - ry * groups_per_row) * PPT;

    uint32_t wc[PPT], wd[PPT], we[PPT], wz[PPT], wn[2 * PPT], wao[PPT], wm[PPT];
    load_words<PPT>(a.color.ptr + (size_t)y * a.color.pitch + (size_t)x0 * 4, wc);
    load_words<PPT>(a.data.ptr + (size_t)y * a.data.pitch + (size_t)x0 * 4, wd);
    load_words<PPT>(a.emission.ptr + (size_t)y * a.emission.pitch + (size_t)x0 * 4, we);
    load_words<PPT>(a.depth.ptr + (size_t)y * a.depth.pitch + (size_t)x0 * 4, wz);
    load_words<2 * PPT>(a.normals.ptr + (size_t)y * a.normals.pitch + (size_t)x0 * 8, wn);
    if (GI == SAH_GI_LPV && a.has_ao) load_words<PPT>(a.ao.ptr + (size_t)y * a.ao.pitch + (size_t)x0 * 4, wao);
    if (SUN == SAH_SHADOW_MODE_RT && a.has_mask) load_words<PPT>(a.shadow_mask.ptr + (size_t)y * a.shadow_mask.pitch + (size_t)x0 * 4, wm);

    uint32_t out[2 * PPT];
#pragma unroll
    for (int i = 0; i < PPT; i++) {
        Px p;
        p.color = wc[i];
        p.data = wd[i];
        p.emission = we[i];
        p.n01 = wn[2 * i];
        p.n23 = wn[2 * i + 1];
        p.depth = __uint_as_float(wz[i]);
        p.ao = (GI == SAH_GI_LPV && a.has_ao) ? __uint_as_float(wao[i]) : 1.0f;
        p.mask = (SUN == SAH_SHADOW_MODE_RT && a.has_mask) ? __uint_as_float(wm[i]) : 1.0f;
        const uint2 r = shade_pixel_general<SUN, GI>(a, csm, lpv, sky, x0 + i, y, p, s_lut);
        out[2 * i] = r.x;
        out[2 * i + 1] = r.y;
    }
    uint8_t* dst = const_cast<uint8_t*>(a.lit.ptr) + (size_t)y * a.lit.pitch + (size_t)x0 * 8;
    if constexpr (PPT == 1) {
        *reinterpret_cast<uint2*>(dst) = make_uint2(out[0], out[1]);
    } else {
        store_words<2 * PPT>(dst, out);
    }
}

// ---- fix-up kernel: general restatement over the deferred pixels -------------------------------------------------------------------
// The fast kernel leaves, per wave, a segment of byte codes (lane * PPT + pixel) and their count (params.hpp: FastArgs).  One
// workgroup takes kFixupSegs consecutive segments, scans their counts in LDS and deals the listed pixels to its threads, so lanes
// stay busy whether a segment holds one stray pixel or is all sky.  No atomics, no list clearing: every wave of the fast kernel
// rewrites its count.
constexpr uint32_t kFixupSegs = 16;
// (at most this many workgroups, striding over the groups of segments: 512 leave an empty list 0.7 us sooner than 2,048, but take
//  3.7 % longer over a frame that lists 29 K pixels — tools/experiments/r5/ab_fixup_grid.sh)
constexpr uint32_t kFixupMaxWorkgroups = 2048;

// One listed pixel, `code` of segment `seg`: back to its place through the map of the fast kernel's thread that listed it, its planes read, shaded
// with the general restatement, stored.  The fix-up kernel's loop body, and the fast kernel's where it finishes its own strays (FastArgs::strays_inline).
template <int SUN, int GI, int PPT, bool SKY_FILL = true>
SAH_DEV void shade_listed_pixel(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const SkyArgs& sky, const FastArgs& f, uint32_t seg,
                                uint32_t code, const float* s_lut) {
    const uint32_t g = seg * 64u + code / PPT;  // the thread of the fast kernel that listed the pixel: the same map back
    const FastPixel at = fast_pixel_of(g, a.width / PPT, a.row_end - a.row_begin, PPT, f.tile_rows, f.row_magic);
    const uint32_t y = a.row_begin + at.row, x = at.x0 + code % PPT;
    Px p;
    p.color = *reinterpret_cast<const uint32_t*>(a.color.ptr + (size_t)y * a.color.pitch + (size_t)x * 4);
    p.data = *reinterpret_cast<const uint32_t*>(a.data.ptr + (size_t)y * a.data.pitch + (size_t)x * 4);
    p.emission = *reinterpret_cast<const uint32_t*>(a.emission.ptr + (size_t)y * a.emission.pitch + (size_t)x * 4);
    p.depth = *reinterpret_cast<const float*>(a.depth.ptr + (size_t)y * a.depth.pitch + (size_t)x * 4);
    const uint2 n = *reinterpret_cast<const uint2*>(a.normals.ptr + (size_t)y * a.normals.pitch + (size_t)x * 8);
    p.n01 = n.x;
    p.n23 = n.y;
    p.ao = (GI == SAH_GI_LPV && a.has_ao) ? *reinterpret_cast<const float*>(a.ao.ptr + (size_t)y * a.ao.pitch + (size_t)x * 4) : 1.0f;
    p.mask = (SUN == SAH_SHADOW_MODE_RT && a.has_mask)
                 ? *reinterpret_cast<const float*>(a.shadow_mask.ptr + (size_t)y * a.shadow_mask.pitch + (size_t)x * 4)
                 : 1.0f;
    const uint2 r = shade_pixel_general<SUN, GI, SKY_FILL>(a, csm, lpv, sky, x, y, p, s_lut);
    *reinterpret_cast<uint2*>(const_cast<uint8_t*>(a.lit.ptr) + (size_t)y * a.lit.pitch + (size_t)x * 8) = r;
}

template <int SUN, int GI, int PPT>
__global__ void __launch_bounds__(256) k_lighting_fixup(const LightingArgs a, const CsmArgs csm, const LpvArgs lpv, const SkyArgs sky,
                                                        const FastArgs f) {
    // nothing listed by any wave (FrameState::deferred_hint): every workgroup leaves here
    if (__hip_atomic_load(&f.state->deferred_hint[f.hint_slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
    // ... and something was: one thread says so in the host's record (StraysRecord) for the 20 K waves of a frame full of strays.  The fast kernel
    // in front of this launch has left its own number in the next launch's word (FrameState::call_no).
    if (blockIdx.x == 0u && threadIdx.x == 0u && f.strays_record)
        __hip_atomic_store(&f.strays_record->listed, f.state->call_no[f.hint_slot ^ 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __shared__ uint32_t s_pref[kFixupSegs + 1];
    __shared__ float s_lut[512];
    stage_format_tables(s_lut, a.luts);
    const uint32_t ngroups = (f.num_segments + kFixupSegs - 1u) / kFixupSegs;
    for (uint32_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    __syncthreads();  // (s_pref of the previous group is read no more; the LUT is in place)
    const uint32_t seg0 = grp * kFixupSegs;
    if (threadIdx.x < 64) {
        const uint32_t lane = threadIdx.x;
        const uint32_t c = (lane < kFixupSegs && seg0 + lane < f.num_segments) ? (uint32_t)f.seg_count[seg0 + lane] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < (int)kFixupSegs; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if ((int)lane >= d) incl += t;
        }
        if (lane < kFixupSegs) s_pref[lane + 1] = incl;
        if (lane == 0) s_pref[0] = 0;
    }
    __syncthreads();
    const uint32_t total = s_pref[kFixupSegs];
    if (total == 0) continue;
    for (uint32_t i = threadIdx.x; i < total; i += 256u) {
        uint32_t s = 0;  // last segment whose prefix is <= i (counts are small: a 4-step search over 16 LDS words)
#pragma unroll
        for (uint32_t step = kFixupSegs / 2; step >= 1; step >>= 1)
            if (s_pref[s + step] <= i) s += step;
        const uint32_t code = f.seg_list[(size_t)(seg0 + s) * f.seg_stride + (i - s_pref[s])];
        shade_listed_pixel<SUN, GI, PPT>(a, csm, lpv, sky, f, seg0 + s, code, s_lut);
    }
    }
}

// ---- LPV gather copy + finiteness scan -----------------------------------------------------------------------------------
// Once per Lighting pass (3 MiB in, 4 MiB out, L2 resident): interleaves the three RGBA16F volumes into 24-byte texels
// {R[4], G[4], B[4]} surrounded by a two-texel border of zeros, and flags inf / NaN texels (feeds the "specular quirk is inert"
// proof).  The fast kernel then gathers one trilinear footprint as 4 (y,z) rows x 48 contiguous bytes = 12 dwordx4 loads touching
// 4-5 cache lines, instead of 24 dwordx2 loads over three allocations, and CLAMP_TO_BORDER needs no per-tap masking: border
// texels are real zeros.
__global__ void __launch_bounds__(256) k_lpv_pack(const VolumeArg r, const VolumeArg g, const VolumeArg b, uint8_t* packed, uint32_t pk_row_pitch,
                                                  uint32_t pk_slice_pitch, FrameState* state) {
    const uint32_t prow = blockIdx.x;  // one block per padded (z, y) row
    const uint32_t ph = r.height + 2 * kLpvPackBorder;
    const uint32_t pz = prow / ph, py = prow - pz * ph;
    const int z = (int)pz - (int)kLpvPackBorder, y = (int)py - (int)kLpvPackBorder;
    const bool row_inside = z >= 0 && z < (int)r.depth && y >= 0 && y < (int)r.height;
    uint32_t bad = 0;
    uint8_t* dst_row = packed + (size_t)pz * pk_slice_pitch + (size_t)py * pk_row_pitch;
    for (uint32_t px = threadIdx.x; px < r.width + 2 * kLpvPackBorder; px += 256) {
        const int x = (int)px - (int)kLpvPackBorder;
        uint2 t[3] = {make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u)};
        if (row_inside && x >= 0 && x < (int)r.width) {
            t[0] = *reinterpret_cast<const uint2*>(r.ptr + (size_t)z * r.slice_pitch + (size_t)y * r.row_pitch + (size_t)x * 8);
            t[1] = *reinterpret_cast<const uint2*>(g.ptr + (size_t)z * g.slice_pitch + (size_t)y * g.row_pitch + (size_t)x * 8);
            t[2] = *reinterpret_cast<const uint2*>(b.ptr + (size_t)z * b.slice_pitch + (size_t)y * b.row_pitch + (size_t)x * 8);
#pragma unroll
            for (int c = 0; c < 3; c++) {  // fp16 exponent all ones <=> inf or NaN
                bad |= ((t[c].x & 0x7c00u) == 0x7c00u) | ((t[c].x & 0x7c000000u) == 0x7c000000u) | ((t[c].y & 0x7c00u) == 0x7c00u) |
                       ((t[c].y & 0x7c000000u) == 0x7c000000u);
            }
        }
        uint2* dst = reinterpret_cast<uint2*>(dst_row + (size_t)px * kLpvPackTexel);
        dst[0] = t[0];
        dst[1] = t[1];
        dst[2] = t[2];
    }
    if (wave_any(bad != 0) && (threadIdx.x & 63) == 0) atomicMax(&state->nonfinite, 1u);
}

// the numerators of lighting_fast.hpp (colx_*_of / rowy_*_of) for every column and row, once per (extent, render resolution, p0, p12, p5, p13):
// columns [0, width) at out (GLSL) and out + stride (Slang), rows [0, height) at out + 2 * stride (GLSL) and out + 2 * stride + row_stride (Slang)
// An entry whose bits are 0x80000000 (-0: a -0 product plus a -0 addend) raises FrameState::colx_neg_zero, which the launcher has cleared: the
// shared-reciprocal divide under FastArgs::pos_div_shared is proven for +0 numerators only.
__global__ void __launch_bounds__(256) k_colx_table(const LightingArgs a, const FastArgs f, float* out, uint32_t stride, uint32_t row_stride) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool neg_zero = false;
    auto put = [&](uint32_t at, float v) {
        out[at] = v;
        neg_zero = neg_zero || __float_as_uint(v) == 0x80000000u;
    };
    if (i < a.width) {
        put(i, colx_glsl_of(a, f, i));
        put(stride + i, colx_slang_of(a, f, i));
    }
    if (i < a.height) {
        put(2u * stride + i, rowy_glsl_of(a, f, i));
        put(2u * stride + row_stride + i, rowy_slang_of(a, f, i));
    }
    if (wave_any(neg_zero) && (threadIdx.x & 63u) == 0u) atomicOr(&f.state->colx_neg_zero, 1u);
}

// surface workgroups per sky workgroup: FastArgs::sky_ratio, chosen by the host with the launch (api.cpp: a whole 4K frame 4 — 1, 2, 8, 16 measured
// worse: DESIGN.md §5 "Deferred pixels ... and the sky" —; small launches fewer, so that a thread of a sky workgroup over an all-sky stretch walks
// fewer pixels one after the other: that walk is the launch's critical path when the launch is short)

// Which bodies of the fast kernel have a twin that finishes its own strays (FINISH; FastArgs::strays_inline): the ones with a sky bound.  The
// general restatement wants 135-207 VGPRs (k_lighting_fixup), and a kernel has one register count.  A SKY body is held at 128 by its launch
// bound, so the finish — a region at the kernel's end, behind a wave-uniform vote, where nothing of the hot path is live — spills what it must,
// where only a wave with strays goes, and the hot path keeps its registers and its occupancy; its uniforms it reads there too (FinishArgs below),
// so that no FINISH body has a private segment or an SGPR spill (profiles/finish_late_kernel_resources.txt).  A body without a sky has no bound: with the
// finish it would take the restatement's count and lose one to five waves per SIMD for every wave of every frame.  Those keep the fix-up launch.
// A twin, not a branch of the one body: compiled into the body that runs in front of a fix-up launch, the finish moved that body's SGPR spills
// and cost it 1.1-1.8 % in every launch, strays or none (profiles/strays_inline_ab.txt).  The body in front of a fix-up launch is the kernel it was.
constexpr bool strays_inline_body(bool sky) { return sky; }

// The finish's view of the fast kernel's five argument blocks.  The general restatement wants nearly every uniform of them (the general matrices
// of the sun and the LPV among them); as kernel arguments they are loaded in the kernel's prologue, for every wave, and kept — spilled to lanes of a
// VGPR — across the hot path that never uses them: 49 SGPR spills in the headline's FINISH body against its twin's 17, and stack slots that left
// the kernel a private segment (36 bytes no instruction touched).  So the finish reads them where it uses them: from the kernarg segment, where
// they lie anyway — no copy, nothing per launch on the host —, through a pointer the optimiser cannot identify with the arguments it has loaded (an
// empty asm statement it cannot see through).  The loads stay scalar loads of the constant address space, and sit behind the listing vote.
// The offsets are the kernel ABI's: explicit arguments in order, each at its natural alignment, from offset 0.
struct FinishArgs {
    const LightingArgs* a;
    const CsmArgs* csm;
    const LpvArgs* lpv;
    const SkyArgs* sky;
    const FastArgs* f;
};
constexpr uint32_t kernarg_align(uint32_t off, uint32_t align) { return (off + align - 1u) / align * align; }
SAH_DEV FinishArgs finish_args_of_fast_kernel() {
    constexpr uint32_t at_a = 0u;
    constexpr uint32_t at_csm = kernarg_align(at_a + (uint32_t)sizeof(LightingArgs), alignof(CsmArgs));
    constexpr uint32_t at_lpv = kernarg_align(at_csm + (uint32_t)sizeof(CsmArgs), alignof(LpvArgs));
    constexpr uint32_t at_sky = kernarg_align(at_lpv + (uint32_t)sizeof(LpvArgs), alignof(SkyArgs));
    constexpr uint32_t at_f = kernarg_align(at_sky + (uint32_t)sizeof(SkyArgs), alignof(FastArgs));
    typedef const __attribute__((address_space(4))) uint8_t* kernarg_ptr;
    kernarg_ptr k = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    FinishArgs r;
    r.a = (const LightingArgs*)(k + at_a);
    r.csm = (const CsmArgs*)(k + at_csm);
    r.lpv = (const LpvArgs*)(k + at_lpv);
    r.sky = (const SkyArgs*)(k + at_sky);
    r.f = (const FastArgs*)(k + at_f);
    return r;
}
// (the argument itself in a body that is not a FINISH body: the same code as before there)
template <bool LATE, class T>
SAH_DEV const T& late_or(const T& arg, const T* late) {
    if constexpr (LATE) return *late;
    else return arg;
}

// ---- fast kernel (per-pixel body: lighting_fast.hpp) ----------------------------------------------------------------------
template <int SUN, int GI, int PPT, bool SKY, bool FINISH = false>
// (106 VGPRs at 4 px/thread = 4 waves per SIMD.  Forcing 5 or 6 with amdgpu_waves_per_eu spills 36-44 bytes per lane and is 12-20 %
// slower, measured.)
// (The sky path — two fp64 transcendentals per pixel — wants 126-137 VGPRs whatever stands next to it, and a kernel has ONE register count: left
// alone the allocator takes 133-137 = 3 waves per SIMD for every wave of the 4- and 2-pixel bodies.  The bound holds every SKY body at four waves
// per SIMD: the 4-pixel body spills 12 bytes of the sky path, the others nothing.  Holding the SKY bodies at their sky-less twins' occupancy (5-8
// waves: 72-96 VGPRs) was built and measured in round 6: the sky path then spills 160-236 bytes per lane and its waves become the launch's tail —
// 1280 x 720 0.0222 -> 0.0380 ms, 4K CSM only 0.118 -> 0.151: tools/experiments/r6/README.md §2.)
__global__ void __launch_bounds__(256, SKY ? 4 : 1) k_lighting_fast(const LightingArgs a, const CsmArgs csm, const LpvArgs lpv, const SkyArgs sky,
                                                                                 const FastArgs f) {
    // Sky.  ProceduralSky::render_sky overwrites lit_scene where depth == 0 (sky_unified.slang:185-206): those pixels need their
    // coordinates and two fp64 transcendentals each, nothing of the surface code.  With a sky bound the first f.sky_first workgroups of the
    // grid are sky workgroups: workgroup i reads the depth of the pixels of surface workgroups [i * sky_ratio, (i + 1) * sky_ratio) and shades
    // the sky among them; surface workgroups leave those pixels alone.  In the same launch the sky's arithmetic fills issue slots the surface
    // waves leave idle (as a kernel of its own behind this one it cost 20 us on the 4 % of sky in the atrium frame: one busy wave per SIMD, in
    // series); leading the grid, the walk is not the launch's tail (api.cpp, where sky_ratio and sky_first are chosen).
    uint32_t block_id = blockIdx.x;
    if (SKY) {
        if (blockIdx.x < f.sky_first) {
            // (a FINISH body's sky workgroup takes its uniforms — the sky block is its alone — where it uses them, like the finish: FinishArgs)
            FinishArgs late = {nullptr, nullptr, nullptr, nullptr, nullptr};
            if constexpr (FINISH) late = finish_args_of_fast_kernel();
            const LightingArgs& wa = late_or<FINISH>(a, late.a);
            const SkyArgs& wsky = late_or<FINISH>(sky, late.sky);
            const FastArgs& wf = late_or<FINISH>(f, late.f);
            const uint32_t ratio = wf.sky_ratio;
            const uint32_t groups_per_row = wa.width / PPT, rows = wa.row_end - wa.row_begin, total = groups_per_row * rows;
#pragma unroll 1
            for (uint32_t k = 0; k < ratio; k++) {
                const uint32_t gid = (blockIdx.x * ratio + k) * 256u + threadIdx.x;
                if (gid >= total) break;
                const FastPixel at = fast_pixel_of(gid, groups_per_row, rows, PPT, wf.tile_rows, wf.row_magic);  // (the surface workgroups' map)
                const uint32_t y = wa.row_begin + at.row, x0 = at.x0;
                uint32_t wz[PPT];
                load_words<PPT>(wa.depth.ptr + (size_t)y * wa.depth.pitch + (size_t)x0 * 4, wz);
#pragma unroll 1
                for (int i = 0; i < PPT; i++) {
                    if (__uint_as_float(wz[i]) != 0.f) continue;
                    Hn lit[4];
                    sky_frag(wa, wsky, x0 + (uint32_t)i, y, lit);
                    *reinterpret_cast<uint2*>(const_cast<uint8_t*>(wa.lit.ptr) + (size_t)y * wa.lit.pitch + (size_t)(x0 + i) * 8) = pack_lit(lit);
                }
            }
            return;
        }
        block_id = blockIdx.x - f.sky_first;
    }
    // the thread's plane loads are requested first: the LUT staging and its barrier below then overlap their latency
    const uint32_t groups_per_row = a.width / PPT;
    const uint32_t gid = block_id * 256u + threadIdx.x;
    const uint32_t rows = a.row_end - a.row_begin;
    const bool active = gid < groups_per_row * rows;
    // which pixels the thread owns: a strip of its row, or — where the launch gathers — its place in the wave's 64-pixel-wide tile (fast_pixel_map.hpp)
    FastPixel at = {0u, 0u};
    if (active) at = fast_pixel_of(gid, groups_per_row, rows, PPT, f.tile_rows, f.row_magic);
    const uint32_t y = a.row_begin + at.row;
    const uint32_t x0 = at.x0;
    const bool lpv_bad = (GI == SAH_GI_LPV) ? (f.state->nonfinite != 0u) : false;
    const bool div_shared = (SUN == SAH_SHADOW_MODE_CSM || GI == SAH_GI_LPV) ? pos_div_shared_of(f) : false;

    // The FINISH body of the traced sun under an LPV at 4 pixels per thread reads each pixel's AO texel where the pixel is shaded: eight planes' texels
    // of four pixels do not fit beside the pixel loop, and its twin spills the AO plane's four words to scratch in the prologue and reloads them for
    // every pixel (20 bytes of private segment, which a FINISH body does not have).  The same texel from the same plane: the same bytes.
    constexpr bool ao_late = FINISH && SUN == SAH_SHADOW_MODE_RT && GI == SAH_GI_LPV && PPT == 4;
    uint32_t wc[PPT], wd[PPT], we[PPT], wz[PPT], wn[2 * PPT], wao[PPT], wm[PPT];
    float colx_g[PPT], colx_s[PPT];
    if (active) {
        load_words<PPT>(a.color.ptr + (size_t)y * a.color.pitch + (size_t)x0 * 4, wc);
        load_words<PPT>(a.data.ptr + (size_t)y * a.data.pitch + (size_t)x0 * 4, wd);
        load_words<PPT>(a.emission.ptr + (size_t)y * a.emission.pitch + (size_t)x0 * 4, we);
        load_words<PPT>(a.depth.ptr + (size_t)y * a.depth.pitch + (size_t)x0 * 4, wz);
        load_words<2 * PPT>(a.normals.ptr + (size_t)y * a.normals.pitch + (size_t)x0 * 8, wn);
        if (GI == SAH_GI_LPV && a.has_ao && !ao_late) load_words<PPT>(a.ao.ptr + (size_t)y * a.ao.pitch + (size_t)x0 * 4, wao);
        if (SUN == SAH_SHADOW_MODE_RT && a.has_mask) load_words<PPT>(a.shadow_mask.ptr + (size_t)y * a.shadow_mask.pitch + (size_t)x0 * 4, wm);
        if (f.colx_tab) {  // (uniform) the per-column numerators of the view-space x: one load instead of PPT IEEE divides
            uint32_t t[PPT];
            if (SUN == SAH_SHADOW_MODE_CSM || GI == SAH_GI_LPV) {
                load_words<PPT>(reinterpret_cast<const uint8_t*>(f.colx_tab + x0), t);
#pragma unroll
                for (int i = 0; i < PPT; i++) colx_g[i] = __uint_as_float(t[i]);
            }
            if (SUN == SAH_SHADOW_MODE_RT) {
                load_words<PPT>(reinterpret_cast<const uint8_t*>(f.colx_tab + f.colx_stride + x0), t);
#pragma unroll
                for (int i = 0; i < PPT; i++) colx_s[i] = __uint_as_float(t[i]);
            }
        }
    }
    __shared__ __attribute__((aligned(16))) float s_lut[TAB_SIZE];
    stage_fast_tables<SUN == SAH_SHADOW_MODE_CSM, GI == SAH_GI_LPV>(s_lut, a, csm, f);
    __syncthreads();
    // each wave's LPV texel box (lighting_fast.hpp: LpvBox): kLpvBoxBytes, 3 KB, per wave beside the table, written and read by that wave alone
    LpvBox box;
    box.lds = nullptr;
    box.valid = false;
    if constexpr (GI == SAH_GI_LPV) {
        __shared__ __attribute__((aligned(16))) uint8_t s_box[4 * kLpvBoxBytes];
        box.lds = s_box + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * kLpvBoxBytes;
    }

    // per-row / per-column terms of the view-space position (two texcoord conventions, see lighting_common.hpp): from the table where
    // the host has built one (uniform branch), else computed
    float rowy_glsl = 0.f, rowy_slang = 0.f;
    if (f.colx_tab) {
        if (SUN == SAH_SHADOW_MODE_CSM || GI == SAH_GI_LPV) rowy_glsl = f.colx_tab[2u * f.colx_stride + y];
        if (SUN == SAH_SHADOW_MODE_RT) rowy_slang = f.colx_tab[2u * f.colx_stride + f.rowy_stride + y];
    } else {
        if (SUN == SAH_SHADOW_MODE_CSM || GI == SAH_GI_LPV) rowy_glsl = rowy_glsl_of(a, f, y);
        if (SUN == SAH_SHADOW_MODE_RT) rowy_slang = rowy_slang_of(a, f, y);
    }

    uint32_t out[2 * PPT];
    uint32_t deferred_mask = 0, sky_mask = 0;
    bool emissive_wave;  // (one vote for the thread's PPT pixels)
    {
        uint32_t any_e = 0;
#pragma unroll
        for (int i = 0; i < PPT; i++) any_e |= we[i];
        emissive_wave = wave_any(active && (any_e & 0xffffffu) != 0u);
    }
#pragma unroll
    for (int i = 0; i < PPT; i++) {
        if (!active) break;
        Px p;
        p.color = wc[i];
        p.data = wd[i];
        p.emission = we[i];
        p.n01 = wn[2 * i];
        p.n23 = wn[2 * i + 1];
        p.depth = __uint_as_float(wz[i]);
        p.ao = (GI == SAH_GI_LPV && a.has_ao) ? __uint_as_float(wao[i]) : 1.0f;
        if constexpr (ao_late) p.ao = a.has_ao ? *reinterpret_cast<const float*>(a.ao.ptr + (size_t)y * a.ao.pitch + (size_t)(x0 + i) * 4) : 1.0f;
        p.mask = (SUN == SAH_SHADOW_MODE_RT && a.has_mask) ? __uint_as_float(wm[i]) : 1.0f;
        const uint32_t x = x0 + i;
        float colx_glsl = 0.f, colx_slang = 0.f;
        if (f.colx_tab) {
            if (SUN == SAH_SHADOW_MODE_CSM || GI == SAH_GI_LPV) colx_glsl = colx_g[i];
            if (SUN == SAH_SHADOW_MODE_RT) colx_slang = colx_s[i];
        } else {
            if (SUN == SAH_SHADOW_MODE_CSM || GI == SAH_GI_LPV) colx_glsl = colx_glsl_of(a, f, x);
            if (SUN == SAH_SHADOW_MODE_RT) colx_slang = colx_slang_of(a, f, x);
        }
        const FastPixelOut r = shade_pixel_fast_sl<SUN, GI>(a, csm, lpv, f, colx_glsl, rowy_glsl, colx_slang, rowy_slang, p, s_lut, lpv_bad, emissive_wave, div_shared, box, i == 0,
                                                                   lpv_box_centre_lane(PPT));
        out[2 * i] = r.lit.x;
        out[2 * i + 1] = r.lit.y;
        if (r.deferred) deferred_mask |= 1u << i;
        if (p.depth == 0.f) sky_mask |= 1u << i;
    }
    if (active) {
        uint8_t* dst = const_cast<uint8_t*>(a.lit.ptr) + (size_t)y * a.lit.pitch + (size_t)x0 * 8;
        if (SKY && sky_mask != 0u) {  // the sky workgroup owns these pixels: per-pixel stores around them
#pragma unroll
            for (int i = 0; i < PPT; i++)
                if (!((sky_mask >> i) & 1u)) *reinterpret_cast<uint2*>(dst + 8 * i) = make_uint2(out[2 * i], out[2 * i + 1]);
        } else if constexpr (PPT == 1) {
            *reinterpret_cast<uint2*>(dst) = make_uint2(out[0], out[1]);
        } else {
            store_words<2 * PPT>(dst, out);
        }
    }
    // deferred pixels -> this wave's segment (no atomics: the wave owns it).  Slots by ballot + mbcnt, one bit plane per pixel of
    // the thread; the order inside a segment is irrelevant.  (Sky pixels are not listed: the sky workgroups find them by their depth.)
    const uint32_t seg = gid >> 6, lane = threadIdx.x & 63u;
    uint32_t front = 0;
    const uint32_t listed = SKY ? deferred_mask & ~sky_mask : deferred_mask;
    if (wave_any(listed != 0u)) {  // (a wave of a coherent frame lists nothing: one vote instead of PPT ballots)
        uint8_t* seg_codes = f.seg_list + (size_t)seg * f.seg_stride;
#pragma unroll
        for (int i = 0; i < PPT; i++) {
            const bool mine = (listed >> i) & 1u;
            const uint64_t m = __ballot(mine);
            if (m) {
                const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (mine) seg_codes[front + before] = (uint8_t)(lane * PPT + (uint32_t)i);
                front += (uint32_t)__builtin_popcountll(m);
            }
        }
        // The FINISH body — the launcher has taken it and enqueues no fix-up launch behind it (FastArgs::strays_inline): the wave shades what it
        // has just listed, dealt densely to its lanes like the fix-up kernel deals a group of segments — n listed pixels are ceil(n / 64) passes.
        // It reads back only its own segment, and overwrites only lit pixels it stored itself: its stores above have to be done first.  A wave's
        // memory operations are in order, and a wave-level fence keeps the compiler from moving a read ahead, as in lpv_box_write(); the wait
        // for the stores' acknowledgements is there besides, in a region that runs for strays only.  (No sky here: the sky workgroups own the
        // depth == 0 pixels of a SKY body.)
        if constexpr (FINISH) {
            static_assert(strays_inline_body(SKY), "no such body");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // (the host's record, StraysRecord: nobody else tells it here.  One store per listing wave of a launch that was predicted to have none)
            const FinishArgs late = finish_args_of_fast_kernel();  // (every uniform of the finish: read here, not in the prologue)
            if (lane == 0u && late.f->strays_record)
                __hip_atomic_store(&late.f->strays_record->listed, late.f->state->call_no[late.f->hint_slot] + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#pragma unroll 1
            for (uint32_t i = lane; i < front; i += 64u)
                shade_listed_pixel<SUN, GI, PPT, false>(*late.a, *late.csm, *late.lpv, *late.sky, *late.f, seg, seg_codes[i], s_lut);
        }
    }
    if (lane == 0 && seg < f.num_segments) {
        f.seg_count[seg] = (uint16_t)front;
        if (front != 0u) f.state->deferred_hint[f.hint_slot] = 1u;  // (see FrameState: the fix-up kernel's workgroups leave at once without it)
    }
    if (gid == 0u) {
        f.state->deferred_hint[f.hint_slot ^ 1u] = 0u;  // the next call's word
        const uint32_t call = f.state->call_no[f.hint_slot] + 1u;  // (FrameState::call_no: this launch's number, and the next launch's word)
        f.state->call_no[f.hint_slot ^ 1u] = call;
        if (f.strays_record) __hip_atomic_store(&f.strays_record->started, call, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
// (re)builds the gather copy of the LPV volumes in front of a Lighting kernel that gathers from it (the fast kernel; the tiled one with f.lpv_fast)
static hipError_t launch_lpv_pack(const LpvArgs& lpv, const FastArgs& f, hipStream_t st) {
    const uint32_t prows = (lpv.red.height + 2 * kLpvPackBorder) * (lpv.red.depth + 2 * kLpvPackBorder);
    const hipError_t me = hipMemsetAsync(&f.state->nonfinite, 0, sizeof(uint32_t), st);  // the new copy's verdict starts at "finite"
    if (me != hipSuccess) return me;
    hipLaunchKernelGGL(k_lpv_pack, dim3(prows), dim3(256), 0, st, lpv.red, lpv.green, lpv.blue, const_cast<uint8_t*>(f.lpv_packed), f.pk_row_pitch,
                       f.pk_slice_pitch, f.state);
    return hipGetLastError();
}
template <int SUN, int GI>
static hipError_t launch_general_ppt(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const SkyArgs& sky, int ppt, hipStream_t st) {
    const uint32_t rows = a.row_end - a.row_begin;
    const uint64_t groups = (uint64_t)(a.width / ppt) * rows;
    if (groups == 0) return hipSuccess;
    const dim3 grid((uint32_t)((groups + 255) / 256)), block(256);
    if (ppt == 4) hipLaunchKernelGGL((k_lighting_general<SUN, GI, 4>), grid, block, 0, st, a, csm, lpv, sky);
    else if (ppt == 2) hipLaunchKernelGGL((k_lighting_general<SUN, GI, 2>), grid, block, 0, st, a, csm, lpv, sky);
    else hipLaunchKernelGGL((k_lighting_general<SUN, GI, 1>), grid, block, 0, st, a, csm, lpv, sky);
    return hipGetLastError();
}

template <int SUN, int GI>
static hipError_t launch_fast_ppt(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const SkyArgs& sky, const FastArgs& f, int ppt,
                                  hipStream_t st) {
    const uint32_t rows = a.row_end - a.row_begin;
    const uint64_t groups = (uint64_t)(a.width / ppt) * rows;
    if (groups == 0) return hipSuccess;
    if (GI == SAH_GI_LPV && f.repack) {
        const hipError_t pe = launch_lpv_pack(lpv, f, st);
        if (pe != hipSuccess) return pe;
    }
    const uint32_t blocks = (uint32_t)((groups + 255) / 256);
    const dim3 block(256);
    auto launch = [&](auto ppt_c) {
        constexpr int P = decltype(ppt_c)::value;
        // (f.sky_first sky workgroups lead the grid: api.cpp)
        if (sky.enabled && f.strays_inline) hipLaunchKernelGGL((k_lighting_fast<SUN, GI, P, true, true>), dim3(f.sky_first + blocks), block, 0, st, a, csm, lpv, sky, f);
        else if (sky.enabled) hipLaunchKernelGGL((k_lighting_fast<SUN, GI, P, true>), dim3(f.sky_first + blocks), block, 0, st, a, csm, lpv, sky, f);
        else hipLaunchKernelGGL((k_lighting_fast<SUN, GI, P, false>), dim3(blocks), block, 0, st, a, csm, lpv, sky, f);
    };
    if (ppt == 4) launch(std::integral_constant<int, 4>{});
    else if (ppt == 2) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 1>{});
    if (f.strays_inline && strays_inline_body(sky.enabled != 0u)) return hipGetLastError();  // the fast kernel has finished its own strays (api.cpp: lighting_strays)
    // (a grid-stride loop over the groups of segments)
    const uint32_t fgroups = (f.num_segments + kFixupSegs - 1) / kFixupSegs;
    const dim3 fgrid(fgroups < kFixupMaxWorkgroups ? fgroups : kFixupMaxWorkgroups);
    if (ppt == 4) hipLaunchKernelGGL((k_lighting_fixup<SUN, GI, 4>), fgrid, block, 0, st, a, csm, lpv, sky, f);
    else if (ppt == 2) hipLaunchKernelGGL((k_lighting_fixup<SUN, GI, 2>), fgrid, block, 0, st, a, csm, lpv, sky, f);
    else hipLaunchKernelGGL((k_lighting_fixup<SUN, GI, 1>), fgrid, block, 0, st, a, csm, lpv, sky, f);
    return hipGetLastError();
}

template <int SUN>
static hipError_t launch_gi(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const SkyArgs& sky, const FastArgs* f, int gi, int ppt,
                            hipStream_t st) {
    switch (gi) {
        case SAH_GI_NONE:
            return f ? launch_fast_ppt<SUN, SAH_GI_NONE>(a, csm, lpv, sky, *f, ppt, st) : launch_general_ppt<SUN, SAH_GI_NONE>(a, csm, lpv, sky, ppt, st);
        case SAH_GI_LPV:
            return f ? launch_fast_ppt<SUN, SAH_GI_LPV>(a, csm, lpv, sky, *f, ppt, st) : launch_general_ppt<SUN, SAH_GI_LPV>(a, csm, lpv, sky, ppt, st);
        default: return hipErrorNotSupported;
    }
}

bool lighting_fast_finishes_strays(bool sky_bound) { return strays_inline_body(sky_bound); }

hipError_t launch_colx_table(const LightingArgs& a, const FastArgs& f, float* out, uint32_t stride, uint32_t row_stride, hipStream_t st) {
    const hipError_t me = hipMemsetAsync(&f.state->colx_neg_zero, 0, sizeof(uint32_t), st);  // the new table's verdict starts at "no -0"
    if (me != hipSuccess) return me;
    hipLaunchKernelGGL(k_colx_table, dim3((max(a.width, a.height) + 255u) / 256u), dim3(256), 0, st, a, f, out, stride, row_stride);
    return hipGetLastError();
}

hipError_t launch_lighting(const LightingArgs& a, const CsmArgs& csm, const LpvArgs& lpv, const CacheArgs& cache, const RtgiArgs& rtgi,
                           const SkyArgs& sky, LightingFamily family, const FastArgs* fast, int sun_mode, int gi, int ppt, bool brute_force_lights,
                           hipStream_t st) {
    // `fast`: what the host established about the uniform blocks (the fast kernel's arguments; for the tiled kernel, when not null, its fast geometry)
    if (family == kLightingTiled) {
        if (gi == SAH_GI_LPV && fast && fast->lpv_fast && fast->repack && a.row_end > a.row_begin) {
            const hipError_t pe = launch_lpv_pack(lpv, *fast, st);
            if (pe != hipSuccess) return pe;
        }
        return launch_lighting_tiled(a, csm, lpv, cache, rtgi, sky, sun_mode, gi, brute_force_lights, fast, st);
    }
    switch (sun_mode) {
        case SAH_SHADOW_MODE_OFF: return launch_gi<SAH_SHADOW_MODE_OFF>(a, csm, lpv, sky, fast, gi, ppt, st);
        case SAH_SHADOW_MODE_CSM: return launch_gi<SAH_SHADOW_MODE_CSM>(a, csm, lpv, sky, fast, gi, ppt, st);
        case SAH_SHADOW_MODE_RT: return launch_gi<SAH_SHADOW_MODE_RT>(a, csm, lpv, sky, fast, gi, ppt, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace sah
