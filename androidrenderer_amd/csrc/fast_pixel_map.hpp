// Which pixels a thread of the fast Lighting kernel owns (lighting.hip: k_lighting_fast's surface workgroups, its sky workgroups' walk, and
// k_lighting_fixup, which turns a listed code back into its pixel).  Integers only, host and device: the host restates nothing, tests/cpp/
// fast_pixel_map_check.cpp compiles this very file.
//
// A launch covers `rows` rows of `gpr` thread groups (gpr = width / ppt; a group is ppt horizontally adjacent pixels, one thread).  Thread
// index gid in [0, gpr * rows) -> (x0, row), a permutation of the groups:
//   tile_rows == 0      linear: row = gid / gpr, x0 = (gid - row * gpr) * ppt.  A wave is a strip of 64 * ppt pixels of one row.
//   tile_rows == R > 0  R = 64 * ppt / kFastTileWidth, a power of two.  The rows are cut into bands of R; band b owns gids [b * R * gpr, (b + 1) * R * gpr),
//                       and since R * gpr is a multiple of 64 (the host requires width % kFastTileWidth == 0) every aligned run of 64 gids — a wave,
//                       and a deferred-pixel segment — lies in one band.  Run t of a band is the tile of kFastTileWidth pixels x R rows at pixel column
//                       t * kFastTileWidth, lanes row-major: lane -> (lane % lpr, lane / lpr) with lpr = kFastTileWidth / ppt lanes per row.  Each row of a
//                       tile is two 128-byte lines of a 4-byte plane and four of normals or lit, so plane loads and lit stores stay whole lines.
//                       (At one pixel per thread R is 1 and the tile is the strip: the map is then the linear one.)
//                       The rows behind the last full band (rows % R of them) keep the linear map on what is left of the gid space.
// The row of gid comes from the multiply-high the linear map already used (row_magic: FastArgs, api.cpp) or the plain divide; the band is a
// mask of it, the rest shifts and masks — no divide by R * gpr, whose magic would leave the multiply-high's < 2^32 bound at 4K.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SAH_PIXEL_MAP_FN __host__ __device__ inline
#else
#define SAH_PIXEL_MAP_FN inline
#endif

namespace sah {

// Width of a wave's tile in pixels.  64 (x 4 rows at 4 pixels per thread) is the shape kept; 16 x 16, 32 x 8 and 128 x 2 were measured beside
// it, each faster than the strip and slower than this one: profiles/fast_tile_map_ab.txt.
constexpr uint32_t kFastTileWidth = 64;

struct FastPixel {
    uint32_t x0, row;  // first pixel of the thread's group; row counted from the launch's first row
};

// rows per tile for `ppt` pixels per thread (what FastArgs::tile_rows holds where the launch is tiled)
SAH_PIXEL_MAP_FN uint32_t fast_tile_rows(uint32_t ppt) { return 64u * ppt / kFastTileWidth; }

// The host's rule (api.cpp: lighting_fast_layout): tiles where the launch gathers — shadow-map taps or the LPV footprint, the accesses whose
// cost follows a wave's footprint in world space —, the width is whole tiles and there is at least one band.  (A launch that gathers nothing only
// streams planes: in 32 x 8 tiles that cost the 4K frame without sun and GI 17 %, in 64 x 4 tiles it is no loss — same file — but those launches were
// not measured beyond that pass and keep their strips.)
SAH_PIXEL_MAP_FN uint32_t fast_tile_rows_for(bool gathers, uint32_t width, uint32_t rows, uint32_t ppt) {
    const uint32_t r = fast_tile_rows(ppt);
    return (gathers && r != 0u && width % kFastTileWidth == 0u && rows >= r) ? r : 0u;
}

SAH_PIXEL_MAP_FN FastPixel fast_pixel_of(uint32_t gid, uint32_t gpr, uint32_t rows, uint32_t ppt, uint32_t tile_rows, uint32_t row_magic) {
    const uint32_t ry = row_magic ? (uint32_t)(((uint64_t)gid * row_magic) >> 32) : gid / gpr;
    FastPixel p;
    const uint32_t band_row = ry & ~(tile_rows - 1u);  // first row of gid's band (tile_rows is a power of two)
    if (tile_rows == 0u || band_row + tile_rows > rows) {  // linear, and the remainder rows of a tiled launch
        p.x0 = (gid - ry * gpr) * ppt;
        p.row = ry;
        return p;
    }
    const uint32_t lpr = kFastTileWidth / ppt;  // lanes per tile row: a power of two
    const uint32_t r = gid - band_row * gpr;
    const uint32_t tile = r >> 6, lane = r & 63u;
    p.x0 = (tile * lpr + (lane & (lpr - 1u))) * ppt;
    p.row = band_row + lane / lpr;
    return p;
}

}  // namespace sah
