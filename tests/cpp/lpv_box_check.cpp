// Checks androidrenderer_amd/csrc/lpv_box.hpp on the host (tests/test_lpv_box_cpu.py builds and runs it; it may also be built with
// -fsanitize=address,undefined and run directly).  For every volume of the list, every reference base r in [0, size + 2]^3 (per axis: the rule is
// separable) and every pixel base in [0, size + 2]:
//   - served <=> both taps of every axis lie inside [o, o + 4);
//   - every staged chunk lies inside the padded allocation, the 96 chunks are the box's 16 (y, z) rows of 96 contiguous bytes, none twice;
//   - every LDS offset a lane reads or writes lies inside the wave's region and is 16-byte aligned, the 96 written chunks tile the region but for the padding behind each z slab,
//     and a served pixel's tap reads the widened bytes of exactly the texel lpv_fetch_packed would load;
//   - the reference lane is a lane of the mask, the one the rule names.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../androidrenderer_amd/csrc/lpv_box.hpp"

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

using namespace sah;

// the rule of one axis: origin, served, clamped offset
void check_axis(uint32_t size) {
    const uint32_t P = lpv_box_padded(size);
    for (uint32_t r = 0; r <= size + 2u; r++) {
        const uint32_t o = lpv_box_origin(r, size);
        CHECK(o + kLpvBoxEdge <= P, "size %u r %u: box [%u, %u) leaves the padded extent %u", size, r, o, o + kLpvBoxEdge, P);
        const int want = (int)r - 1 < 0 ? 0 : ((int)r - 1 > (int)P - 4 ? (int)P - 4 : (int)r - 1);
        CHECK((int)o == want, "size %u r %u: origin %u, clamp(r - 1, 0, P - 4) is %d", size, r, o, want);
        // the reference lane itself is always served
        CHECK(lpv_box_served(lpv_box_delta(r, o), 0u, 0u), "size %u: the reference base %u is not served by its own box at %u", size, r, o);
        for (uint32_t base = 0; base <= size + 2u; base++) {
            const uint32_t d = lpv_box_delta(base, o);
            const bool taps_inside = base >= o && base + 1u < o + kLpvBoxEdge;
            CHECK(lpv_box_served(d, 0u, 0u) == taps_inside && lpv_box_served(0u, d, 0u) == taps_inside && lpv_box_served(0u, 0u, d) == taps_inside,
                  "size %u r %u base %u: served %d, taps inside %d", size, r, base, (int)lpv_box_served(d, 0u, 0u), (int)taps_inside);
            const uint32_t c = lpv_box_clamp_delta(d);
            CHECK(c <= 2u && (!taps_inside || c == d), "size %u r %u base %u: clamped offset %u", size, r, base, c);
        }
    }
}

// staging and taps of one volume: pitches as ctx_cache.hpp lays the copy out (+ 64 bytes of slack behind it)
void check_volume(uint32_t w, uint32_t h, uint32_t d) {
    const uint32_t size[3] = {w, h, d};
    const uint64_t row_pitch = (uint64_t)lpv_box_padded(w) * kLpvBoxSrcTexel, slice_pitch = row_pitch * lpv_box_padded(h);
    const uint64_t bytes = slice_pitch * lpv_box_padded(d) + 64u;
    std::printf("volume %u x %u x %u: padded %u x %u x %u, %llu bytes\n", w, h, d, lpv_box_padded(w), lpv_box_padded(h), lpv_box_padded(d),
                (unsigned long long)bytes);
    for (int axis = 0; axis < 3; axis++) check_axis(size[axis]);
    // every reference base: every staged chunk inside the padded allocation
    for (uint32_t rx = 0; rx <= w + 2u; rx++)
        for (uint32_t ry = 0; ry <= h + 2u; ry++)
            for (uint32_t rz = 0; rz <= d + 2u; rz++) {
                const uint32_t ox = lpv_box_origin(rx, w), oy = lpv_box_origin(ry, h), oz = lpv_box_origin(rz, d);
                for (uint32_t c = 0; c < kLpvBoxChunks; c++) {
                    const uint64_t src = lpv_box_chunk_src(c, ox, oy, oz, (uint32_t)row_pitch, (uint32_t)slice_pitch);
                    CHECK(src + 16u <= bytes - 64u, "r (%u, %u, %u): chunk %u ends at %llu of %llu", rx, ry, rz, c, (unsigned long long)src + 16u,
                          (unsigned long long)bytes - 64u);
                }
            }
    // the layout in detail: every reference base on the corners and edges, and a walk through the interior
    std::vector<uint32_t> rs[3];
    for (int axis = 0; axis < 3; axis++)
        for (uint32_t r = 0; r <= size[axis] + 2u; r++)
            if (r < 4u || r + 4u > size[axis] + 2u || r % 7u == 0u) rs[axis].push_back(r);
    std::vector<int> owner(kLpvBoxBytes);
    for (uint32_t rx : rs[0])
        for (uint32_t ry : rs[1])
            for (uint32_t rz : rs[2]) {
                const uint32_t ox = lpv_box_origin(rx, w), oy = lpv_box_origin(ry, h), oz = lpv_box_origin(rz, d);
                owner.assign(kLpvBoxBytes, -1);
                for (uint32_t c = 0; c < kLpvBoxChunks; c++) {
                    const uint64_t src = lpv_box_chunk_src(c, ox, oy, oz, (uint32_t)row_pitch, (uint32_t)slice_pitch);
                    CHECK(src + 16u <= bytes - 64u, "chunk %u of the box at (%u, %u, %u) ends at %llu of %llu", c, ox, oy, oz, (unsigned long long)src + 16u,
                          (unsigned long long)bytes - 64u);
                    const uint32_t row = c / kLpvBoxChunksPerRow, j = c % kLpvBoxChunksPerRow;
                    const uint64_t row_src = (uint64_t)(oz + row / 4u) * slice_pitch + (uint64_t)(oy + row % 4u) * row_pitch + (uint64_t)ox * kLpvBoxSrcTexel;
                    CHECK(src == row_src + 16u * j, "chunk %u: source %llu is not byte %u of its row at %llu", c, (unsigned long long)src, 16u * j,
                          (unsigned long long)row_src);
                    const uint32_t dst = lpv_box_chunk_dst(c);
                    CHECK(dst % 16u == 0u && dst + 32u <= kLpvBoxBytes, "chunk %u: LDS offset %u", c, dst);
                    CHECK(dst == 2u * (uint32_t)(src - row_src) + (row / 4u) * kLpvBoxSlab + (row % 4u) * kLpvBoxRow,
                          "chunk %u: LDS offset %u is not twice its offset in the row", c, dst);
                    for (uint32_t b = dst; b < dst + 32u && b < kLpvBoxBytes; b++) {
                        CHECK(owner[b] < 0, "LDS byte %u written by chunks %d and %u", b, owner[b], c);
                        owner[b] = (int)c;
                    }
                }
                // every byte is written but the 16 bytes of padding behind each z slab, which no tap reads (owner -1 below)
                for (uint32_t b = 0; b < kLpvBoxBytes; b++)
                    CHECK((owner[b] >= 0) == (b % kLpvBoxSlab < kLpvBoxEdge * kLpvBoxRow), "LDS byte %u: written by chunk %d", b, owner[b]);
                // taps: every clamped offset; texel (o + dx + xs, o + dy + yy, o + dz + zz) of the copy is where lpv_fetch_packed loads it from
                for (uint32_t dz = 0; dz <= 2u; dz++)
                    for (uint32_t dy = 0; dy <= 2u; dy++)
                        for (uint32_t dx = 0; dx <= 2u; dx++) {
                            const uint32_t base = lpv_box_lds_base(dx, dy, dz);
                            for (uint32_t k = 0; k < 4u; k++)
                                for (uint32_t xs = 0; xs < 2u; xs++)
                                    for (uint32_t ch = 0; ch < 3u; ch++) {
                                        const uint32_t at = base + lpv_box_lds_row(k) + xs * kLpvBoxTexel + 16u * ch;
                                        CHECK(at % 16u == 0u && at + 16u <= kLpvBoxBytes, "tap at (%u, %u, %u) row %u: LDS offset %u", dx, dy, dz, k, at);
                                        if (at + 16u > kLpvBoxBytes) continue;
                                        CHECK(owner[at] >= 0 && owner[at + 15u] == owner[at], "tap at (%u, %u, %u) row %u reads LDS bytes no chunk wrote", dx, dy, dz, k);
                                        if (owner[at] < 0) continue;
                                        // the copy's byte this LDS quad widens: chunk source + half the offset inside the chunk's 32 bytes
                                        const uint32_t c = (uint32_t)owner[at];
                                        const uint64_t src = lpv_box_chunk_src(c, ox, oy, oz, (uint32_t)row_pitch, (uint32_t)slice_pitch) + (at - lpv_box_chunk_dst(c)) / 2u;
                                        const uint64_t want = (uint64_t)(oz + dz + (k >> 1)) * slice_pitch + (uint64_t)(oy + dy + (k & 1u)) * row_pitch +
                                                              (uint64_t)(ox + dx + xs) * kLpvBoxSrcTexel + 8u * ch;
                                        CHECK(src == want, "tap at (%u, %u, %u) row %u x %u channel %u reads copy byte %llu, lpv_fetch_packed loads %llu", dx, dy, dz, k,
                                              xs, ch, (unsigned long long)src, (unsigned long long)want);
                                    }
                        }
            }
}

void check_reference_lane() {
    const uint32_t centres[3] = {lpv_box_centre_lane(4), lpv_box_centre_lane(2), lpv_box_centre_lane(1)};
    CHECK(centres[0] == 40u && centres[1] == 48u && centres[2] == 32u, "centre lanes %u %u %u", centres[0], centres[1], centres[2]);
    uint64_t m = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < 4000; i++) {
        m ^= m << 13, m ^= m >> 7, m ^= m << 17;
        uint64_t act = i % 5 == 0 ? 1ull << (m & 63u) : (i % 5 == 1 ? m & (m >> 21) & (m << 9) : m);
        if (i == 0) act = ~0ull;
        if (act == 0ull) continue;
        for (uint32_t centre : centres) {
            const uint32_t ref = lpv_box_reference_lane(act, centre);
            CHECK(ref < 64u && ((act >> ref) & 1ull), "mask %016llx: reference lane %u is not in it", (unsigned long long)act, ref);
            uint32_t want = 64u;
            for (uint32_t l = centre; l < 64u && want == 64u; l++)
                if ((act >> l) & 1ull) want = l;
            for (int l = (int)centre - 1; l >= 0 && want == 64u; l--)
                if ((act >> l) & 1ull) want = (uint32_t)l;
            CHECK(ref == want, "mask %016llx centre %u: reference lane %u, expected %u", (unsigned long long)act, centre, ref, want);
        }
    }
}

}  // namespace

int main() {
    static_assert(kLpvBoxBytes == 3136 && kLpvBoxBytes % 16 == 0 && kLpvBoxChunks == 96 && kLpvBoxChunks <= 64 + 32, "a lane stages chunks lane and 64 + (lane & 31)");
    check_volume(32, 32, 32);
    check_volume(128, 32, 32);
    check_volume(1, 1, 1);
    check_reference_lane();
    if (g_failures) {
        std::printf("%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("lpv_box ok\n");
    return 0;
}
