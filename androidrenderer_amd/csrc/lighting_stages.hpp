// The stages of sah_lighting that digest the descriptor into kernel-argument blocks, for the entry points that share them: sah_lighting
// (api.cpp, where they are defined) and sah_lighting_vrs (api_vrs.cpp).  Each validates its part, fills the block it is given and returns a
// sah_status; none touches device memory or a cache of the context.
#pragma once
#include <stdint.h>

#include "../../include/sah_hip.h"
#include "params.hpp"

struct sah_ctx;  // ctx.hpp

namespace sah {

// What the stages of one call share about it
struct LightingCall {
    uint32_t W, H, r0, r1;  // extent of lit, output rows [r0, r1)
    uint32_t sun_mode, gi_kind;
    bool vec4ok;  // width, addresses and pitches of every plane allow 16-byte accesses (four pixels per thread)
};

// Targets and G-buffer: validation, the row range, the planes, the view and the sun constants
int lighting_targets(sah_ctx* ctx, const sah_lighting_desc* d, LightingCall& call, LightingArgs& a);
// The sun's cascaded shadow map (all zero for another shadow mode)
int lighting_csm(sah_ctx* ctx, const sah_lighting_desc* d, const LightingCall& call, CsmArgs& csm);
// Its two parts that another pass sampling the cascades with shadow_pcf() shares (sah_sun_shafts): the constants of the D16 conversion, and
// what the sun's constants alone decide, the split depths and biasMat * cascade_matrices[c]
void csm_d16_conversion(CsmArgs& csm);
void csm_sun_tables(const sah_sun_light_constants& sun, CsmArgs& csm);
// The LPV overlay (all zero for another GI kind)
int lighting_gi_lpv(sah_ctx* ctx, const sah_lighting_desc* d, const LightingCall& call, LpvArgs& lpv);
// The sky fill (all zero without a sky)
int lighting_sky(sah_ctx* ctx, const sah_lighting_desc* d, SkyArgs& sky);

}  // namespace sah
