// C ABI: the mip-chain generator (include/sah_mip_chain.h; kernel in mip_chain.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/sah_mip_chain.h"
#include "ctx.hpp"
#include "launch.hpp"

namespace {
// the kernel variant of a (source, destination) format pair, or -1
int pair_kind(uint32_t src, uint32_t dst) {
    if ((src == SAH_FORMAT_D32_SFLOAT || src == SAH_FORMAT_R32_SFLOAT) && dst == SAH_FORMAT_R32_SFLOAT) return sah::kMipChainR32Min;
    if (src == SAH_FORMAT_R16_SFLOAT && dst == src) return sah::kMipChainR16;
    if (src == SAH_FORMAT_R16G16B16A16_SFLOAT && dst == src) return sah::kMipChainRGBA16;
    if (src == SAH_FORMAT_B10G11R11_UFLOAT_PACK32 && dst == src) return sah::kMipChainR11G11B10;
    return -1;
}
// extent, pitch and alignment of a plane whose format is already known to be one of the pairs'
bool plane_laid_out(const sah_plane& p) {
    const uint32_t texel = format_bpp(p.format);
    return p.width && p.height && (uint64_t)p.row_pitch_bytes >= (uint64_t)p.width * texel && ((uintptr_t)p.ptr % texel) == 0 && (p.row_pitch_bytes % texel) == 0;
}
}  // namespace

extern "C" int sah_mip_chain_generate(sah_ctx* ctx, const sah_plane* src, const sah_plane* dst_levels, uint32_t num_dst_levels) {
    SAH_RANGE();
    if (!ctx) return SAH_ERR_INVALID_ARGUMENT;
    if (!src || !src->ptr || !dst_levels) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: null source or level array");
    if (num_dst_levels == 0 || num_dst_levels > SAH_MIP_CHAIN_MAX_LEVELS) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: 1..12 levels");
    for (uint32_t i = 0; i < num_dst_levels; i++)
        if (!dst_levels[i].ptr) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: level %u has no memory", i);
    const int kind = pair_kind(src->format, dst_levels[0].format);
    if (kind < 0) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "mip_chain_generate: formats %u -> %u are none of the four pairs", src->format, dst_levels[0].format);
    for (uint32_t i = 1; i < num_dst_levels; i++)
        if (dst_levels[i].format != dst_levels[0].format) return fail(ctx, SAH_ERR_UNSUPPORTED_FORMAT, "mip_chain_generate: level %u has another format than level 0", i);
    if (!plane_laid_out(*src)) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: the source's extent, pitch or alignment");
    if (src->width > SAH_MIP_CHAIN_MAX_SOURCE || src->height > SAH_MIP_CHAIN_MAX_SOURCE)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: a source larger than 4096 needs more than SPD's 12 levels");
    const uint32_t w0 = dst_levels[0].width, h0 = dst_levels[0].height;
    for (uint32_t i = 0; i < num_dst_levels; i++) {
        if (!plane_laid_out(dst_levels[i])) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: level %u: extent, pitch or alignment", i);
        if (dst_levels[i].width != std::max(1u, w0 >> i) || dst_levels[i].height != std::max(1u, h0 >> i))
            return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: level %u is not max(1, level 0 >> %u)", i, i);
    }
    // SpdSetup, ffx_spd.h:334-349
    const uint32_t groups_x = (src->width + 63) / 64, groups_y = (src->height + 63) / 64;
    const uint32_t mips = (uint32_t)std::min(std::floor(std::log2((float)std::max(src->width, src->height))), 12.0f);
    if (mips > 1 && num_dst_levels == 1) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: %u levels are made and there is no level 1 for the missing ones", mips);
    if (mips >= 7 && num_dst_levels < 6) return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: %u levels are made and level 5 is missing", mips);
    if (mips < 7 && num_dst_levels < mips && groups_x * groups_y > 1)
        return fail(ctx, SAH_ERR_INVALID_ARGUMENT, "mip_chain_generate: missing levels below 6 with more than one workgroup");

    sah::MipChainArgs a = {};
    a.src = parg(src);
    a.src_w = src->width, a.src_h = src->height;
    a.inv_w = 1.0f / (float)src->width, a.inv_h = 1.0f / (float)src->height;  // invInputSize = vec2(1.f) / textureSize(imgSrc, 0)
    for (uint32_t i = 0; i < SAH_MIP_CHAIN_MAX_LEVELS; i++) {
        // mip_chain_generator.cpp:109-124: the level's own view, or level 1's from mipLevels on.  (With one level nothing is aimed at slots >= 1.)
        a.slot[i] = parg(&dst_levels[i < num_dst_levels ? i : std::min(1u, num_dst_levels - 1)]);
        a.slot_w[i] = std::max(1u, w0 >> i), a.slot_h[i] = std::max(1u, h0 >> i);
    }
    a.mips = mips;
    a.num_workgroups = groups_x * groups_y;
    a.counter = ctx->mip_chain_counter.word;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, sah_guard_touch(ctx, ctx->guard_mip_chain));
    HIP_TRY(ctx, hipMemsetAsync(a.counter, 0, sizeof(uint32_t), ctx->stream));  // "Clear counter", mip_chain_generator.cpp:63-77
    HIP_TRY(ctx, sah::launch_mip_chain(a, (sah::MipChainKind)kind, ctx->stream));
    return SAH_OK;
}
