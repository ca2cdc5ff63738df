// C ABI: the post chain — copy scene, bloom, tonemap (kernels in post.hip, tonemap.hip, tonemap_tol.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/sah_hip.h"
#include "ctx.hpp"
#include "launch.hpp"

namespace {
// Output code of the tonemap tail for one channel value x = colour * luma/(luma+1):
// pow(x, 1/2.2) (fp32 result of the fp64 libm value), then the sRGB OETF the swap chain applies, then UNORM8
// (scene_upsample.frag:66-72 + hardware sRGB write; DESIGN.md "Numerics").  Monotone non-decreasing in x.
uint32_t tonemap_code(float x) {
    if (!(x > 0.0f)) return 0u;
    const float g = (float)std::pow((double)x, (double)(1.f / 2.2f));
    if (!(g > 0.0f)) return 0u;
    if (g >= 1.0f) return 255u;
    const double d = (double)g;
    const float s = (float)((d <= 0.0031308) ? 12.92 * d : 1.055 * std::pow(d, 1.0 / 2.4) - 0.055);
    if (!(s > 0.0f)) return 0u;
    if (s >= 1.0f) return 255u;
    return (uint32_t)(s * 255.0f + 0.5f);
}
// thr[k] = smallest positive float whose code is >= k, found by bisection on the bit pattern (positive floats order like
// their bits); thr[0] is never read.
void build_tonemap_thresholds(float thr[256]) {
    thr[0] = 0.0f;
    for (uint32_t k = 1; k < 256; k++) {
        uint32_t lo = 0u, hi = 0x7f800000u;  // code(+0) = 0 < k <= 255 = code(+inf)
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            float f;
            memcpy(&f, &mid, 4);
            if (tonemap_code(f) >= k) hi = mid; else lo = mid;
        }
        memcpy(&thr[k], &hi, 4);
    }
}
// First-level table of the device's code search: bucket b holds the positive floats whose bit pattern >> kTmBucketShift equals
// base + b (16 buckets per octave, from thr[1] to thr[255]); first[b] = min(code(first float of the bucket), 252).  A bucket spans at
// most three codes (checked), so code(x) = first[b] + [x >= thr[first + 1]] + [x >= thr[first + 2]] + [x >= thr[first + 3]].
bool build_tonemap_buckets(const float thr[256], uint8_t first[sah::kTmMaxBuckets], uint32_t* base, uint32_t* count) {
    uint32_t tb[256];
    memcpy(tb, thr, sizeof(tb));
    const uint32_t b0 = tb[1] >> sah::kTmBucketShift, b1 = tb[255] >> sah::kTmBucketShift;
    const uint32_t n = b1 - b0 + 1;
    if (n > sah::kTmMaxBuckets) return false;
    auto code_of_bits = [&](uint32_t bits) {  // number of thresholds <= the float
        uint32_t c = 0;
        for (uint32_t k = 1; k < 256; k++) c += tb[k] <= bits ? 1u : 0u;
        return c;
    };
    for (uint32_t b = 0; b < n; b++) {
        const uint32_t start = (b0 + b) << sah::kTmBucketShift, end = ((b0 + b + 1) << sah::kTmBucketShift) - 1u;
        // bucket 0 also takes everything below thr[1] (clamped there by the kernel): code 0
        const uint32_t lo = b == 0 ? 0u : code_of_bits(start);
        const uint32_t f = lo < 252u ? lo : 252u;
        if (code_of_bits(end) - f > 3u) return false;
        first[b] = (uint8_t)f;
    }
    for (uint32_t b = n; b < sah::kTmMaxBuckets; b++) first[b] = 252;
    *base = b0;
    *count = n;
    return true;
}

// ---- sah_tonemap_ex, stage by stage: arguments, code tables, axis tables, launch ----
// checks the arguments (in the order, and with the messages, callers see) and fills everything of `t` that they alone decide
int tonemap_args(sah_ctx* ctx, const sah_plane* scene, const sah_mipchain* bloom, const sah_plane* out, uint32_t row_begin, uint32_t row_end, uint32_t flags,
                 sah::TonemapArgs& t) {
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (flags & ~SAH_TONEMAP_TOLERANCE_1CODE) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "unknown tonemap flags %#x", flags);
    if (!rgba16f_ok(scene) || !bloom || bloom->num_mips > SAH_MAX_BLOOM_MIPS || !out || !out->ptr)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "tonemap needs scene, bloom chain and output");
    if (out->format != SAH_FORMAT_R8G8B8A8_SRGB && out->format != SAH_FORMAT_R8G8B8A8_UNORM)
        return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "tonemap output must be R8G8B8A8");
    if ((uint64_t)out->row_pitch_bytes < (uint64_t)out->width * 4 || ((uintptr_t)out->ptr % 4) || (out->row_pitch_bytes % 4))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bad output pitch/alignment");
    if (row_begin == 0 && row_end == 0) row_end = out->height;
    if (row_end > out->height || row_begin > row_end) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bad row range");
    memset(&t, 0, sizeof(t));
    t.scene = parg(scene);
    t.scene_w = scene->width;
    t.scene_h = scene->height;
    t.num_mips = bloom->num_mips;
    for (uint32_t m = 0; m < bloom->num_mips; m++) {
        if (!rgba16f_ok(&bloom->mips[m])) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "bloom mip %u must be RGBA16F", m);
        t.mips[m] = parg(&bloom->mips[m]);
        t.mip_w[m] = bloom->mips[m].width;
        t.mip_inv_w[m] = 1.0f / (float)bloom->mips[m].width;
        t.mip_inv_h[m] = 1.0f / (float)bloom->mips[m].height;
        t.mip_h[m] = bloom->mips[m].height;
    }
    for (uint32_t m = bloom->num_mips; m < 6; m++) {  // the kernel's staging loads are unconditional: absent mips alias the scene (nothing of them is used)
        t.mips[m] = t.scene;
        t.mip_w[m] = scene->width;
        t.mip_h[m] = scene->height;
    }
    t.out = parg(out);
    t.out_w = out->width;
    t.out_h = out->height;
    t.row_begin = row_begin;
    t.row_end = row_end;
    return SAH_OK;
}

// the code search's two device tables, built once per context (~15k libm pow calls)
int ensure_tonemap_code_tables(sah_ctx* ctx) {
    if (ctx->tm_codes.ready()) return SAH_OK;
    struct {
        float thr[256];
        uint8_t first[sah::kTmMaxBuckets];
    } tab;
    uint32_t bucket_base = 0, bucket_count = 0;
    build_tonemap_thresholds(tab.thr);
    if (!build_tonemap_buckets(tab.thr, tab.first, &bucket_base, &bucket_count))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "tonemap code table: a bucket spans more than three codes (internal)");
    // the same two-level search with one read per look-up: per bucket the three thresholds behind its first code, and that code
    float code_tab[sah::kTmMaxBuckets][4];
    for (uint32_t b = 0; b < sah::kTmMaxBuckets; b++) {
        const uint32_t f = tab.first[b];  // <= 252
        code_tab[b][0] = tab.thr[f + 1];
        code_tab[b][1] = tab.thr[f + 2];
        code_tab[b][2] = tab.thr[f + 3];
        memcpy(&code_tab[b][3], &f, 4);
    }
    // both tables are uploaded into locals and published together: a context whose second upload failed must not be left with the
    // first table set and the second one null (the next call would skip this stage and launch with a null code table)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float *d_thr = nullptr, *d_code = nullptr;
    hipError_t e = hipMalloc((void**)&d_thr, sizeof(tab));
    if (e == hipSuccess) e = hipMemcpy(d_thr, &tab, sizeof(tab), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&d_code, sizeof(code_tab));
    if (e == hipSuccess) e = hipMemcpy(d_code, code_tab, sizeof(code_tab), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d_thr) (void)hipFree(d_thr);
        if (d_code) (void)hipFree(d_code);
        return fail(ctx, SAH_ERR_HIP, "tonemap code tables: %s", hipGetErrorString(e));
    }
    ctx->tm_codes.publish(ctx->cache_epoch, d_thr, d_code, bucket_base, bucket_count, tab.thr[1], tab.thr[255]);
    return SAH_OK;
}

// per-column / per-row axis set-ups of the tolerance composite: a function of the extents only, kept across calls
int tonemap_axis_tables(sah_ctx* ctx, const sah_mipchain* bloom, const sah_plane* out, sah::TonemapArgs& t) {
    uint32_t key[2 + 2 * 8 + 1] = {out->width, out->height};
    for (uint32_t m = 0; m < bloom->num_mips; m++) {
        key[2 + 2 * m] = bloom->mips[m].width;
        key[3 + 2 * m] = bloom->mips[m].height;
    }
    key[18] = bloom->num_mips;
    t.axis_stride = (std::max(out->width, out->height) + 63u) & ~63u;
    const size_t need = (size_t)6 * 2 * 4 * t.axis_stride * sizeof(sah::TmAxis);
    bool rebuild = false;
    HIP_TRY(ctx, ctx->tm_axis.prepare(ctx->stream, ctx->cache_epoch, need, key, sizeof(key), false, &rebuild));
    t.axis_tables = (const sah::TmAxis*)ctx->tm_axis.buf.ptr;
    if (rebuild) {
        HIP_TRY(ctx, sah::launch_tonemap_axis_tables(t, (sah::TmAxis*)ctx->tm_axis.buf.ptr, ctx->stream));
        ctx->tm_axis.built(ctx->cache_epoch, key, sizeof(key));
    }
    return SAH_OK;
}

int tonemap_launch(sah_ctx* ctx, const sah::TonemapArgs& t, bool tolerance) {
    if (tolerance) HIP_TRY(ctx, sah::launch_tonemap_tol(t, ctx->stream));
    else HIP_TRY(ctx, sah::launch_tonemap(t, ctx->stream));
    return SAH_OK;
}
}  // namespace

extern "C" {

int sah_copy_scene_rows(sah_ctx* ctx, const sah_plane* lit, const sah_plane* out, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!rgba16f_ok(lit) || !rgba16f_ok(out)) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "copy_scene needs RGBA16F planes");
    if (row_begin == 0 && row_end == 0) row_end = out->height;
    if (row_end > out->height || row_begin > row_end) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bad row range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah::launch_copy_scene(parg(lit), lit->width, lit->height, parg(out), out->width, out->height, row_begin, row_end, ctx->stream));
    return SAH_OK;
}

int sah_copy_scene(sah_ctx* ctx, const sah_plane* lit, const sah_plane* out) { return sah_copy_scene_rows(ctx, lit, out, 0, 0); }

static int bloom_range(sah_ctx* ctx, const sah_plane* scene, const sah_mipchain* bloom, uint32_t first_mip, uint32_t last_mip, uint32_t row_begin,
                       uint32_t row_end) {
    if ((first_mip == 0 && !rgba16f_ok(scene)) || !bloom || bloom->num_mips == 0 || bloom->num_mips > SAH_MAX_BLOOM_MIPS)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bloom needs an RGBA16F scene and 1..%d mips", SAH_MAX_BLOOM_MIPS);
    for (uint32_t m = 0; m < bloom->num_mips; m++)
        if (!rgba16f_ok(&bloom->mips[m])) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "bloom mip %u must be RGBA16F", m);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (uint32_t m = first_mip; m <= last_mip && m < bloom->num_mips; m++) {  // bloomer.cpp:50-151: scene -> mip0, mip i -> mip i+1
        const sah_plane* src = m == 0 ? scene : &bloom->mips[m - 1];
        const sah_plane* dst = &bloom->mips[m];
        const uint32_t r0 = m == first_mip ? row_begin : 0u, r1 = m == first_mip ? row_end : dst->height;
        // the small mips of the chain, two per launch (post.hip: k_bloom_pair): whole mips only, and only where the texels of the first
        // one that neighbouring tiles compute twice cost less than the launch they save (mip 2 and beyond of a 4K chain)
        const bool whole = r0 == 0 && r1 == dst->height;
        if (whole && m + 1 <= last_mip && m + 1 < bloom->num_mips && (uint64_t)dst->width * dst->height <= (1u << 18)) {
            const sah_plane* nxt = &bloom->mips[m + 1];
            hipError_t e = hipSuccess;
            if (sah::launch_bloom_pair(parg(src), src->width, src->height, parg(dst), dst->width, dst->height, parg(nxt), nxt->width, nxt->height, ctx->stream, &e)) {
                HIP_TRY(ctx, e);
                m++;
                continue;
            }
        }
        HIP_TRY(ctx, sah::launch_bloom_downsample(parg(src), src->width, src->height, parg(dst), dst->width, dst->height, r0, r1, ctx->stream));
    }
    return SAH_OK;
}

// "Copy scene" + the first bloom dispatch in one pass over lit_scene (post.hip: k_copy_bloom_mip0).  Rows of `antialiased` that the fused
// launch cannot own (farther than 3 rows from the rows of mip 0's sources) are copied by plain launches; extents that do not suit it take
// the two passes one after the other.
int sah_copy_scene_bloom_mip0_rows(sah_ctx* ctx, const sah_plane* lit, const sah_plane* out, const sah_mipchain* bloom, uint32_t aa_row_begin, uint32_t aa_row_end,
                                   uint32_t mip_row_begin, uint32_t mip_row_end) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!rgba16f_ok(lit) || !rgba16f_ok(out)) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "copy_scene needs RGBA16F planes");
    if (!bloom || bloom->num_mips == 0 || bloom->num_mips > SAH_MAX_BLOOM_MIPS || !rgba16f_ok(&bloom->mips[0]))
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bloom needs 1..%d RGBA16F mips", SAH_MAX_BLOOM_MIPS);
    const sah_plane* m0 = &bloom->mips[0];
    if (aa_row_begin == 0 && aa_row_end == 0) aa_row_end = out->height;
    if (mip_row_begin == 0 && mip_row_end == 0) mip_row_end = m0->height;
    if (aa_row_end > out->height || aa_row_begin > aa_row_end || mip_row_end > m0->height || mip_row_begin > mip_row_end)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bad row range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (mip_row_end > mip_row_begin && aa_row_end > aa_row_begin) {
        // what the fused launch can own: from 3 rows above the first source row of the mip rows to 3 rows below the last
        const uint32_t lo = (uint32_t)std::max<int64_t>(std::max<int64_t>((int64_t)2 * mip_row_begin - 3, (int64_t)aa_row_begin), 0);
        const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)2 * mip_row_end + 2, aa_row_end);
        if (hi > lo) {
            hipError_t e = hipSuccess;
            if (sah::launch_copy_bloom_mip0(parg(lit), lit->width, lit->height, parg(out), out->width, out->height, parg(m0), m0->width, m0->height, mip_row_begin,
                                            mip_row_end, lo, hi, ctx->stream, &e)) {
                HIP_TRY(ctx, e);
                if (lo > aa_row_begin) HIP_TRY(ctx, sah::launch_copy_scene(parg(lit), lit->width, lit->height, parg(out), out->width, out->height, aa_row_begin, lo, ctx->stream));
                if (aa_row_end > hi) HIP_TRY(ctx, sah::launch_copy_scene(parg(lit), lit->width, lit->height, parg(out), out->width, out->height, hi, aa_row_end, ctx->stream));
                return SAH_OK;
            }
        }
    }
    // the two passes
    if (aa_row_end > aa_row_begin)
        HIP_TRY(ctx, sah::launch_copy_scene(parg(lit), lit->width, lit->height, parg(out), out->width, out->height, aa_row_begin, aa_row_end, ctx->stream));
    if (mip_row_end > mip_row_begin)
        HIP_TRY(ctx, sah::launch_bloom_downsample(parg(out), out->width, out->height, parg(m0), m0->width, m0->height, mip_row_begin, mip_row_end, ctx->stream));
    return SAH_OK;
}

int sah_bloom(sah_ctx* ctx, const sah_plane* scene, const sah_mipchain* bloom) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!bloom || bloom->num_mips == 0) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bloom needs 1..%d mips", SAH_MAX_BLOOM_MIPS);
    return bloom_range(ctx, scene, bloom, 0, bloom->num_mips - 1, 0, bloom->mips[0].height);
}

int sah_bloom_mip0_rows(sah_ctx* ctx, const sah_plane* scene, const sah_mipchain* bloom, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!bloom || bloom->num_mips == 0) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bloom needs 1..%d mips", SAH_MAX_BLOOM_MIPS);
    if (row_end > bloom->mips[0].height || row_begin > row_end) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bad mip 0 row range");
    return bloom_range(ctx, scene, bloom, 0, 0, row_begin, row_end);
}

int sah_bloom_from_mip0(sah_ctx* ctx, const sah_plane* scene, const sah_mipchain* bloom) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!bloom || bloom->num_mips == 0) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bloom needs 1..%d mips", SAH_MAX_BLOOM_MIPS);
    if (bloom->num_mips == 1) return SAH_OK;
    return bloom_range(ctx, scene, bloom, 1, bloom->num_mips - 1, 0, bloom->mips[1].height);
}

int sah_bloom_mip_rows(sah_ctx* ctx, const sah_plane* scene, const sah_mipchain* bloom, uint32_t mip, uint32_t row_begin, uint32_t row_end) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!bloom || bloom->num_mips == 0 || bloom->num_mips > SAH_MAX_BLOOM_MIPS || mip >= bloom->num_mips)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bloom needs 1..%d mips and a mip index below their number", SAH_MAX_BLOOM_MIPS);
    if (row_end > bloom->mips[mip].height || row_begin > row_end) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bad row range");
    return bloom_range(ctx, scene, bloom, mip, mip, row_begin, row_end);
}

int sah_bloom_from_mip(sah_ctx* ctx, const sah_plane* scene, const sah_mipchain* bloom, uint32_t mip) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!bloom || bloom->num_mips == 0 || bloom->num_mips > SAH_MAX_BLOOM_MIPS || mip >= bloom->num_mips)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "bloom needs 1..%d mips and a mip index below their number", SAH_MAX_BLOOM_MIPS);
    if (mip + 1 >= bloom->num_mips) return SAH_OK;
    return bloom_range(ctx, scene, bloom, mip + 1, bloom->num_mips - 1, 0, bloom->mips[mip + 1].height);
}

int sah_bloom_source_rows(uint32_t src_height, uint32_t dst_height, uint32_t row_begin, uint32_t row_end, uint32_t out[2]) {
    if (!out || src_height == 0 || dst_height == 0 || row_begin > row_end || row_end > dst_height) return SAH_ERR_INVALID_ARGUMENT;
    out[0] = out[1] = 0;
    if (row_begin == row_end) return SAH_OK;
    // exact integer floors of c -+ 2 with c = ((2 j + 1) * hs - hd) / (2 hd); with hs = 2 hd every tap coordinate is an integer + 0.5 and no
    // rounding can move its floor, otherwise one row of slack either side (androidrenderer_amd/shard.py: _downsample_sources)
    const int64_t hs = src_height, hd = dst_height, slack = (hs == 2 * hd) ? 0 : 1;
    auto floordiv = [](int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    const int64_t lo = floordiv((2 * (int64_t)row_begin + 1) * hs - hd - 4 * hd, 2 * hd) - slack;
    const int64_t hi = floordiv((2 * ((int64_t)row_end - 1) + 1) * hs - hd + 4 * hd, 2 * hd) + 1 + slack + 1;
    out[0] = (uint32_t)std::min<int64_t>(std::max<int64_t>(lo, 0), hs);
    out[1] = (uint32_t)std::min<int64_t>(std::max<int64_t>(hi, 0), hs);
    return SAH_OK;
}

int sah_tonemap(sah_ctx* ctx, const sah_plane* scene, const sah_mipchain* bloom, const sah_plane* out, uint32_t row_begin, uint32_t row_end) {
    return sah_tonemap_ex(ctx, scene, bloom, out, row_begin, row_end, 0u);
}

int sah_tonemap_ex(sah_ctx* ctx, const sah_plane* scene, const sah_mipchain* bloom, const sah_plane* out, uint32_t row_begin, uint32_t row_end,
                   uint32_t flags) {
    SAH_RANGE();
    sah::TonemapArgs t;
    if (const int rc = tonemap_args(ctx, scene, bloom, out, row_begin, row_end, flags, t); rc != SAH_OK) return rc;
    if (const int rc = ensure_tonemap_code_tables(ctx); rc != SAH_OK) return rc;
    t.thresholds = ctx->tm_codes.thresholds;
    t.code_table = ctx->tm_codes.code_table;
    t.bucket_base = ctx->tm_codes.bucket_base;
    t.thr_lo = ctx->tm_codes.thr_lo;
    t.thr_hi = ctx->tm_codes.thr_hi;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_tonemap));
    // (the tolerance kernel stages six mips; a longer chain takes the strict kernel, whose result is inside the tolerance by definition)
    bool tol_ok = (flags & SAH_TONEMAP_TOLERANCE_1CODE) && bloom->num_mips <= 6;
    for (uint32_t m = 0; m < bloom->num_mips; m++) tol_ok = tol_ok && bloom->mips[m].width <= 65536u && bloom->mips[m].height <= 65536u;  // (16-bit extents in its LDS table)
    if (tol_ok) {
        if (const int rc = tonemap_axis_tables(ctx, bloom, out, t); rc != SAH_OK) return rc;
    }
    return tonemap_launch(ctx, t, tol_ok);
}

}  // extern "C"
