// Checks androidrenderer_amd/csrc/fast_pixel_map.hpp on the host (tests/test_fast_pixel_map_cpu.py builds and runs it; it may also be built
// with -fsanitize=address,undefined and run directly).  For every shape of the list:
//   - the map is a bijection of [0, gpr * rows) onto the thread groups (x0 a multiple of ppt below the width, row below rows, none twice);
//   - with tile_rows 0 it is the linear split, and with the multiply-high it equals the plain divide;
//   - every aligned run of 64 gids inside the tiled region is exactly a kFastTileWidth-pixel x tile_rows-row rectangle, lanes row-major;
//   - the rows behind the last full band are mapped linearly.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../androidrenderer_amd/csrc/fast_pixel_map.hpp"

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (g_failures++ < 20) {              \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);         \
                std::printf("\n");                \
            }                                     \
        }                                         \
    } while (0)

// api.cpp: lighting_fast_layout
uint32_t row_magic_of(uint64_t gpr, uint64_t rows) {
    const uint64_t threads = (gpr * rows + 255) / 256 * 256;
    return (gpr >= 2 && threads * gpr < (1ull << 32)) ? (uint32_t)((1ull << 32) / gpr) + 1u : 0u;
}

// `tiled`: take the host's rule for a gathering launch; else tile_rows 0.  `expect_magic` / `expect_rows`: what the shape is in the list for.
void check_shape(uint32_t width, uint32_t rows, uint32_t ppt, bool tiled, int expect_magic, int expect_rows) {
    const uint32_t gpr = width / ppt, total = gpr * rows;
    const uint32_t magic = row_magic_of(gpr, rows);
    const uint32_t R = tiled ? sah::fast_tile_rows_for(true, width, rows, ppt) : 0u;
    std::printf("%u x %u at %u px/thread: tile_rows %u, row_magic %s\n", width, rows, ppt, R, magic ? "yes" : "no");
    if (expect_magic >= 0) CHECK((magic != 0u) == (expect_magic != 0), "%ux%u ppt %u: row_magic %u", width, rows, ppt, magic);
    if (expect_rows >= 0) CHECK(R == (uint32_t)expect_rows, "%ux%u ppt %u: tile_rows %u, expected %d", width, rows, ppt, R, expect_rows);
    CHECK(sah::fast_tile_rows_for(false, width, rows, ppt) == 0u, "a launch that does not gather is tiled");
    const uint32_t lpr = sah::kFastTileWidth / ppt;
    const uint32_t full_rows = R ? rows / R * R : 0u;  // the tiled region: whole bands
    if (R) CHECK((uint64_t)gpr * R % 64u == 0u, "a band is not whole waves");
    std::vector<uint8_t> seen(total, 0);
    for (uint32_t gid = 0; gid < total; gid++) {
        const sah::FastPixel p = sah::fast_pixel_of(gid, gpr, rows, ppt, R, magic);
        const sah::FastPixel q = sah::fast_pixel_of(gid, gpr, rows, ppt, R, 0u);
        CHECK(p.x0 == q.x0 && p.row == q.row, "gid %u: multiply-high (%u, %u) against divide (%u, %u)", gid, p.x0, p.row, q.x0, q.row);
        CHECK(p.row < rows && p.x0 < width && p.x0 % ppt == 0u, "gid %u -> (%u, %u) outside", gid, p.x0, p.row);
        if (p.row >= rows || p.x0 >= width) continue;
        const uint32_t group = p.row * gpr + p.x0 / ppt;
        CHECK(!seen[group], "gid %u: group (%u, %u) owned twice", gid, p.x0, p.row);
        seen[group] = 1;
        if (gid >= full_rows * gpr) {  // linear: all of it with tile_rows 0, the remainder rows otherwise
            CHECK(p.row == gid / gpr && p.x0 == (gid % gpr) * ppt, "gid %u: (%u, %u) is not the linear split", gid, p.x0, p.row);
        } else {  // lane of a tile: against the first lane of its aligned run of 64
            const sah::FastPixel o = sah::fast_pixel_of(gid & ~63u, gpr, rows, ppt, R, magic);
            const uint32_t lane = gid & 63u;
            CHECK(o.x0 % sah::kFastTileWidth == 0u && o.row % R == 0u, "gid %u: tile origin (%u, %u) not aligned", gid, o.x0, o.row);
            CHECK(p.x0 == o.x0 + (lane % lpr) * ppt && p.row == o.row + lane / lpr, "gid %u: lane %u at (%u, %u), tile at (%u, %u)", gid, lane, p.x0, p.row,
                  o.x0, o.row);
            CHECK(lane / lpr < R, "gid %u: lane %u below the tile", gid, lane);
        }
    }
    for (uint32_t g = 0; g < total; g++) CHECK(seen[g], "group %u of %ux%u ppt %u owned by nobody", g, width, rows, ppt);
}

}  // namespace

int main() {
    static_assert(sah::kFastTileWidth == 64, "the expected tile_rows below are those of 64-pixel tiles: 4 / 2 / 1 rows at 4 / 2 / 1 pixels per thread");
    check_shape(3840, 2160, 4, true, 1, 4);   // the headline: 3840 x 2160 at 4 pixels per thread
    check_shape(3840, 291, 1, true, 1, 1);    // either side of the multiply-high's limit (threads * gpr < 2^32)
    check_shape(3840, 292, 1, true, 0, 1);
    check_shape(3840, 291, 2, true, 1, 2);    // (the same rows in tiles of two rows: one row behind the last full band at 291)
    check_shape(3840, 4663, 4, true, 0, 4);   // past the limit at 4 pixels per thread (960 groups per row), three rows behind the last full band
    check_shape(64, 16, 4, true, -1, 4);
    check_shape(64, 16, 2, true, -1, 2);
    check_shape(64, 16, 1, true, -1, 1);
    check_shape(128, 23, 4, true, -1, 4);     // three rows behind the last full band
    check_shape(128, 21, 4, true, -1, 4);     // one row
    check_shape(128, 21, 2, true, -1, 2);     // one row
    check_shape(128, 21, 1, true, -1, 1);     // none: a tile of one row is the strip
    check_shape(96, 21, 4, true, -1, 0);      // 96 % 64 != 0: linear by the host's rule
    check_shape(96, 21, 2, true, -1, 0);
    check_shape(96, 21, 1, true, -1, 0);
    check_shape(64, 4, 4, true, -1, 4);       // 16 groups x 4 rows: a single tile
    check_shape(32, 8, 4, true, -1, 0);       // 8 groups x 8 rows: narrower than a tile
    check_shape(64, 3, 4, true, -1, 0);       // rows < R: the host's rule says linear ...
    check_shape(72, 16, 4, true, -1, 0);      // 72 % 64 != 0: linear by the host's rule
    check_shape(72, 16, 4, false, -1, 0);     // tile_rows 0
    check_shape(3840, 2160, 4, false, 1, 0);  // tile_rows 0 at the headline: the linear split with the multiply-high
    {  // ... and a launch whose rows are ALL remainder, map forced on: still the linear split
        const uint32_t gpr = 16, rows = 3, ppt = 4, R = 4;
        for (uint32_t gid = 0; gid < gpr * rows; gid++) {
            const sah::FastPixel p = sah::fast_pixel_of(gid, gpr, rows, ppt, R, row_magic_of(gpr, rows));
            CHECK(p.row == gid / gpr && p.x0 == (gid % gpr) * ppt, "all-remainder gid %u -> (%u, %u)", gid, p.x0, p.row);
        }
    }
    if (g_failures) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("fast_pixel_map ok\n");
    return 0;
}
