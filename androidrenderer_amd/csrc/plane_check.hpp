// Host-side argument rules of the screen-space passes: what a plane must look like, which bytes it covers, how many texels a launch can
// index and what a row window means.  Plain C++ over the C ABI's structs, nothing of HIP: tests/cpp/plane_check.cpp builds it stand-alone.
// The rasteriser, the ray tracer, Lighting and the mip chain check their planes by OTHER rules (one status for everything, alignment to the
// texel: api_raster.cpp, api_rt.cpp, api.cpp, api_mip_chain.cpp); those are not copies of this one and are not to be merged into it.
#pragma once
#include <cstdint>

#include "../../include/sah_rtgi_denoise.h"  // (sah_hip.h, and the two formats only that pass accepts)

inline uint32_t format_bpp(uint32_t f) {
    switch (f) {
        case SAH_FORMAT_R8_UNORM: return 1;
        case SAH_FORMAT_R16_SFLOAT: case SAH_FORMAT_D16_UNORM: return 2;
        case SAH_FORMAT_R8G8B8A8_UNORM: case SAH_FORMAT_R8G8B8A8_SRGB: case SAH_FORMAT_R16G16_SFLOAT: case SAH_FORMAT_R32_SFLOAT:
        case SAH_FORMAT_B10G11R11_UFLOAT_PACK32: case SAH_FORMAT_D32_SFLOAT: return 4;
        case SAH_FORMAT_R16G16B16A16_SFLOAT: case SAH_FORMAT_R32G32_SFLOAT: return 8;
        case SAH_FORMAT_R32G32B32A32_SFLOAT: return 16;
    }
    return 0;
}

inline bool plane_ok(const sah_plane* p, uint32_t fmt_a, uint32_t fmt_b, uint32_t w, uint32_t h) {
    if (!p || !p->ptr) return false;
    if (p->format != fmt_a && p->format != fmt_b) return false;
    if (p->width != w || p->height != h) return false;
    return (uint64_t)p->row_pitch_bytes >= (uint64_t)w * format_bpp(p->format);
}

inline bool rgba16f_ok(const sah_plane* p) {
    return p && p->ptr && p->format == SAH_FORMAT_R16G16B16A16_SFLOAT && p->width && p->height &&
           (uint64_t)p->row_pitch_bytes >= (uint64_t)p->width * 8 && ((uintptr_t)p->ptr % 8) == 0 && (p->row_pitch_bytes % 8) == 0;
}

// The plane rule of the screen-space passes.  SAH_OK, or: a null plane or pointer is SAH_ERR_INVALID_ARGUMENT; then another format than
// `format` is SAH_ERR_UNSUPPORTED_FORMAT, whatever else is wrong; then an empty extent, a pitch below a row, or a pointer or pitch that is
// no multiple of 4 (whatever the texel size) is SAH_ERR_INVALID_ARGUMENT.
inline int plane_status(const sah_plane* p, uint32_t format) {
    if (!p || !p->ptr) return SAH_ERR_INVALID_ARGUMENT;
    if (p->format != format) return SAH_ERR_UNSUPPORTED_FORMAT;
    if (!p->width || !p->height || (uint64_t)p->row_pitch_bytes < (uint64_t)p->width * format_bpp(format) || ((uintptr_t)p->ptr % 4) || (p->row_pitch_bytes % 4))
        return SAH_ERR_INVALID_ARGUMENT;
    return SAH_OK;
}

struct PlaneSpec {
    const sah_plane* p;
    uint32_t format;
    const char* name;  // the argument and its format, for the message: "depth (D32_SFLOAT)"
};
// the status of the first of `n` planes that breaks the rule, and its index in *bad; SAH_OK when none does
inline int planes_status(const PlaneSpec* specs, int n, int* bad) {
    for (int i = 0; i < n; i++)
        if (const int rc = plane_status(specs[i].p, specs[i].format); rc != SAH_OK) {
            *bad = i;
            return rc;
        }
    return SAH_OK;
}

// The bytes a buffer covers, [begin, end).  Unsigned 64-bit and wrapping on purpose: callers hand in any address, and a range whose end
// wraps past zero compares the way it always has.
struct ByteRange {
    uintptr_t begin, end;
};
// of a plane that passed plane_status: up to the end of its last row, not of that row's pitch
inline ByteRange byte_range(const sah_plane* p) {
    const uintptr_t b = (uintptr_t)p->ptr;
    return {b, b + (uint64_t)(p->height - 1) * p->row_pitch_bytes + (uint64_t)p->width * format_bpp(p->format)};
}
inline ByteRange byte_range(const void* p, uint64_t bytes) { return {(uintptr_t)p, (uintptr_t)p + bytes}; }
inline bool overlaps(const ByteRange& a, const ByteRange& b) { return a.begin < b.end && b.begin < a.end; }

// an extent of 2^31 or more, or 2^32 texels or more: beyond what the kernels' 32-bit coordinates and texel indices hold
inline bool texel_count_too_large(uint32_t w, uint32_t h) { return ((w | h) >> 31) || (uint64_t)w * h >= (1ull << 32); }

// The row window [row_begin, row_end) of an h-row target: (0, 0) means all rows.  False for a window that ends beyond h or before it begins;
// an empty one (row_begin == row_end != 0) is fine.
inline bool resolve_rows(uint32_t* row_begin, uint32_t* row_end, uint32_t h) {
    if (*row_begin == 0 && *row_end == 0) *row_end = h;
    return *row_end <= h && *row_begin <= *row_end;
}
