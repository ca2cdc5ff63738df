// Checks androidrenderer_amd/csrc/plane_check.hpp on the host (tests/test_plane_check_cpu.py builds it with -fsanitize=address,undefined and runs
// it).  Nothing of HIP is included and no address below is ever dereferenced: the planes point at made-up addresses.
//   - plane_status for every format format_bpp knows: null plane, null pointer, another format, empty extents, pitch one byte below / exactly a
//     row, pointer off by 1, 2, 3, a pitch that is no multiple of 4, an R16_SFLOAT row of odd width; a format error beats a layout error;
//   - planes_status: the first offender's index and status;
//   - byte_range / overlaps: 1 x 1, touching, one shared byte, the gap behind a pitched plane's last row, a range whose end wraps;
//   - texel_count_too_large and resolve_rows at their boundaries.
#include <cstdint>
#include <cstdio>

#include "../../androidrenderer_amd/csrc/plane_check.hpp"

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

const uint32_t kFormats[] = {SAH_FORMAT_R8_UNORM, SAH_FORMAT_R8G8B8A8_UNORM, SAH_FORMAT_R8G8B8A8_SRGB, SAH_FORMAT_R16_SFLOAT,
                             SAH_FORMAT_R16G16_SFLOAT, SAH_FORMAT_R16G16B16A16_SFLOAT, SAH_FORMAT_R32_SFLOAT, SAH_FORMAT_B10G11R11_UFLOAT_PACK32,
                             SAH_FORMAT_D16_UNORM, SAH_FORMAT_D32_SFLOAT, SAH_FORMAT_R32G32_SFLOAT, SAH_FORMAT_R32G32B32A32_SFLOAT};
const uint32_t kBpp[] = {1, 4, 4, 2, 4, 8, 4, 4, 2, 4, 8, 16};
constexpr int kNumFormats = sizeof(kFormats) / sizeof(kFormats[0]);

sah_plane plane(uintptr_t address, uint32_t w, uint32_t h, uint32_t pitch, uint32_t format) {
    sah_plane p;
    p.ptr = reinterpret_cast<void*>(address);
    p.width = w, p.height = h, p.row_pitch_bytes = pitch, p.format = format;
    return p;
}

void check_plane_status() {
    const uintptr_t base = 0x10000;
    CHECK(format_bpp(0) == 0 && format_bpp(13) == 0, "an unknown format has a texel size");
    for (int f = 0; f < kNumFormats; f++) {
        const uint32_t fmt = kFormats[f], bpp = kBpp[f], other = kFormats[(f + 1) % kNumFormats];
        CHECK(format_bpp(fmt) == bpp, "format %u: %u bytes per texel, not %u", fmt, format_bpp(fmt), bpp);
        const uint32_t w = 8, row = w * bpp;  // a multiple of 4 for every format
        const sah_plane good = plane(base, w, 3, row, fmt);
        CHECK(plane_status(&good, fmt) == SAH_OK, "format %u: a tight plane is refused", fmt);
        CHECK(plane_status(nullptr, fmt) == SAH_ERR_INVALID_ARGUMENT, "format %u: null plane", fmt);
        sah_plane p = good;
        p.ptr = nullptr;
        CHECK(plane_status(&p, fmt) == SAH_ERR_INVALID_ARGUMENT, "format %u: null ptr", fmt);
        CHECK(plane_status(&p, other) == SAH_ERR_INVALID_ARGUMENT, "format %u: null ptr comes before the format", fmt);
        CHECK(plane_status(&good, other) == SAH_ERR_UNSUPPORTED_FORMAT, "format %u taken for %u", fmt, other);
        p = good, p.width = 0;
        CHECK(plane_status(&p, fmt) == SAH_ERR_INVALID_ARGUMENT, "format %u: width 0", fmt);
        p = good, p.height = 0;
        CHECK(plane_status(&p, fmt) == SAH_ERR_INVALID_ARGUMENT, "format %u: height 0", fmt);
        p = good, p.row_pitch_bytes = row - 1;
        CHECK(plane_status(&p, fmt) == SAH_ERR_INVALID_ARGUMENT, "format %u: pitch one byte below a row", fmt);
        if (row > 4) {  // ... and when that is not also a misaligned pitch: 4 bytes below
            p = good, p.row_pitch_bytes = row - 4;
            CHECK(plane_status(&p, fmt) == SAH_ERR_INVALID_ARGUMENT, "format %u: pitch four bytes below a row", fmt);
        }
        p = good, p.row_pitch_bytes = row + 4;
        CHECK(plane_status(&p, fmt) == SAH_OK, "format %u: pitch of a row and 4 bytes", fmt);
        for (uintptr_t off = 1; off < 4; off++) {
            p = good, p.ptr = reinterpret_cast<void*>(base + off);
            CHECK(plane_status(&p, fmt) == SAH_ERR_INVALID_ARGUMENT, "format %u: pointer off by %u", fmt, (unsigned)off);
        }
        p = good, p.ptr = reinterpret_cast<void*>(base + 4);  // 4-byte alignment is enough, whatever the texel
        CHECK(plane_status(&p, fmt) == SAH_OK, "format %u: pointer off by 4", fmt);
        p = good, p.row_pitch_bytes = row + 2;
        CHECK(plane_status(&p, fmt) == SAH_ERR_INVALID_ARGUMENT, "format %u: pitch %u is no multiple of 4", fmt, row + 2);
        // both the format and the layout wrong: the format speaks
        p = good, p.width = 0, p.row_pitch_bytes = 3, p.ptr = reinterpret_cast<void*>(base + 1);
        CHECK(plane_status(&p, other) == SAH_ERR_UNSUPPORTED_FORMAT, "format %u: a format error must come before a layout error", fmt);
    }
    // a 2-byte format whose exact row is no multiple of 4: refused, and accepted once the pitch is rounded up
    sah_plane odd = plane(base, 5, 2, 10, SAH_FORMAT_R16_SFLOAT);
    CHECK(plane_status(&odd, SAH_FORMAT_R16_SFLOAT) == SAH_ERR_INVALID_ARGUMENT, "R16_SFLOAT, width 5, pitch 10 is accepted");
    odd.row_pitch_bytes = 12;
    CHECK(plane_status(&odd, SAH_FORMAT_R16_SFLOAT) == SAH_OK, "R16_SFLOAT, width 5, pitch 12 is refused");
    // a row of 2^32 bytes and more does not wrap into a small one
    const sah_plane wide = plane(base, 0x80000000u, 1, 16, SAH_FORMAT_R16G16B16A16_SFLOAT);
    CHECK(plane_status(&wide, SAH_FORMAT_R16G16B16A16_SFLOAT) == SAH_ERR_INVALID_ARGUMENT, "a 2^34-byte row fits a pitch of 16");

    // the first offender of a list, by index
    const sah_plane a = plane(base, 4, 4, 16, SAH_FORMAT_D32_SFLOAT), b = plane(base, 4, 4, 15, SAH_FORMAT_D32_SFLOAT);
    const PlaneSpec specs[4] = {{&a, SAH_FORMAT_D32_SFLOAT, "a"}, {&a, SAH_FORMAT_R32_SFLOAT, "a as R32"}, {&b, SAH_FORMAT_D32_SFLOAT, "b"}, {nullptr, 0, "null"}};
    int bad = -1;
    CHECK(planes_status(specs, 1, &bad) == SAH_OK && bad == -1, "one good plane: bad = %d", bad);
    CHECK(planes_status(specs, 0, &bad) == SAH_OK && bad == -1, "no plane: bad = %d", bad);
    CHECK(planes_status(specs, 4, &bad) == SAH_ERR_UNSUPPORTED_FORMAT && bad == 1, "four planes: bad = %d", bad);
    CHECK(planes_status(specs + 2, 2, &bad) == SAH_ERR_INVALID_ARGUMENT && bad == 0, "the last two: bad = %d", bad);
}

void check_byte_ranges() {
    const uint32_t RGBA16F = SAH_FORMAT_R16G16B16A16_SFLOAT;
    const uintptr_t base = 0x20000;
    // 1 x 1: its texel, whatever the pitch
    const sah_plane one = plane(base, 1, 1, 4096, RGBA16F);
    const ByteRange r1 = byte_range(&one);
    CHECK(r1.begin == base && r1.end == base + 8, "1 x 1 RGBA16F covers [%#llx, %#llx)", (unsigned long long)r1.begin, (unsigned long long)r1.end);
    CHECK(overlaps(r1, r1), "a plane does not overlap itself");
    // every format's texel size reaches the range
    for (int f = 0; f < kNumFormats; f++) {
        const sah_plane p = plane(base, 3, 2, 64, kFormats[f]);
        CHECK(byte_range(&p).end == base + 64 + 3 * kBpp[f], "format %u: 3 x 2 at pitch 64 ends at +%llu", kFormats[f], (unsigned long long)(byte_range(&p).end - base));
    }
    // touching end to begin; sharing one byte
    const sah_plane a = plane(base, 4, 4, 32, RGBA16F);  // tight: [base, base + 128)
    const sah_plane touching = plane(base + 128, 4, 4, 32, RGBA16F), before = plane(base - 128, 4, 4, 32, RGBA16F);
    CHECK(byte_range(&a).end == base + 128, "a tight 4 x 4 RGBA16F plane ends at +%llu", (unsigned long long)(byte_range(&a).end - base));
    CHECK(!overlaps(byte_range(&a), byte_range(&touching)) && !overlaps(byte_range(&touching), byte_range(&a)), "planes that touch end to begin overlap");
    CHECK(!overlaps(byte_range(&a), byte_range(&before)) && !overlaps(byte_range(&before), byte_range(&a)), "planes that touch begin to end overlap");
    const ByteRange last_byte = byte_range(reinterpret_cast<const void*>(base + 127), 1), next_byte = byte_range(reinterpret_cast<const void*>(base + 128), 1);
    CHECK(overlaps(byte_range(&a), last_byte) && overlaps(last_byte, byte_range(&a)), "a plane and its last byte do not overlap");
    CHECK(!overlaps(byte_range(&a), next_byte), "a plane and the byte behind it overlap");
    const ByteRange shared = byte_range(reinterpret_cast<const void*>(base + 127), 64);  // (a buffer need not be aligned to be compared)
    CHECK(overlaps(byte_range(&a), shared) && overlaps(shared, byte_range(&a)), "two ranges that share one byte do not overlap");
    // a pitched plane: the last row ends short of height * pitch, and a neighbour may start in the tail of that gap
    const sah_plane pitched = plane(base, 4, 4, 64, RGBA16F);  // rows of 32 bytes at pitch 64: [base, base + 3 * 64 + 32)
    CHECK(byte_range(&pitched).end == base + 224, "a pitched plane ends at +%llu", (unsigned long long)(byte_range(&pitched).end - base));
    const sah_plane in_tail = plane(base + 224, 4, 1, 32, RGBA16F), in_row_gap = plane(base + 32, 4, 1, 32, RGBA16F);
    CHECK(!overlaps(byte_range(&pitched), byte_range(&in_tail)), "a neighbour in the gap behind the last row overlaps");
    CHECK(overlaps(byte_range(&pitched), byte_range(&in_row_gap)), "a neighbour in the gap behind the FIRST row does not overlap (the range is one interval)");
    const sah_plane tail_minus_4 = plane(base + 220, 4, 1, 32, RGBA16F);
    CHECK(overlaps(byte_range(&pitched), byte_range(&tail_minus_4)), "a neighbour that starts in the last row's last texel does not overlap");
    // The top of the address space: a 1024 x 1 RGBA16F plane 4096 bytes below 2^64 covers 8192 bytes, and its end wraps to 4096.  By the same
    // unsigned arithmetic, begin < end fails for it, so that:
    const uintptr_t top = (uintptr_t)0 - 4096;
    const sah_plane wrapping = plane(top, 1024, 1, 8192, RGBA16F);
    const ByteRange rw = byte_range(&wrapping);
    CHECK(rw.begin == top && rw.end == 4096, "the wrapping plane covers [%#llx, %#llx)", (unsigned long long)rw.begin, (unsigned long long)rw.end);
    CHECK(!overlaps(rw, rw), "top < 4096: a wrapped range overlaps itself");                                                    // top < 4096 is false
    CHECK(!overlaps(rw, byte_range(reinterpret_cast<const void*>(256), 256)), "a wrapped range overlaps [256, 512)");          // top < 512 is false
    CHECK(!overlaps(rw, byte_range(reinterpret_cast<const void*>(top + 1024), 1024)), "a wrapped range overlaps what lies inside it");  // top + 1024 < 4096 is false
    CHECK(overlaps(byte_range(reinterpret_cast<const void*>(top), 4095), byte_range(reinterpret_cast<const void*>(top + 1024), 1024)),
          "a range that ends one byte below 2^64 does not overlap what lies inside it");
    const ByteRange to_zero = byte_range(reinterpret_cast<const void*>(top), 4096);  // ends at 2^64, which is 0
    CHECK(to_zero.end == 0 && !overlaps(to_zero, byte_range(reinterpret_cast<const void*>(top + 1024), 1024)), "a range that ends at 2^64 overlaps");
}

void check_texel_count() {
    CHECK(!texel_count_too_large(65536, 65535), "65536 x 65535 is too large");
    CHECK(texel_count_too_large(65536, 65536), "65536 x 65536 is not too large");
    CHECK(texel_count_too_large(1, 0x80000000u) && texel_count_too_large(0x80000000u, 1), "1 x 2^31 is not too large");
    CHECK(!texel_count_too_large(0x7fffffffu, 1) && !texel_count_too_large(1, 0x7fffffffu), "(2^31 - 1) x 1 is too large");
    CHECK(!texel_count_too_large(0x7fffffffu, 2) && texel_count_too_large(0x7fffffffu, 3), "(2^31 - 1) x 2 and x 3");
}

void check_rows() {
    const uint32_t h = 37;
    uint32_t b = 0, e = 0;
    CHECK(resolve_rows(&b, &e, h) && b == 0 && e == h, "(0, 0) of %u rows became (%u, %u)", h, b, e);
    b = h, e = h;
    CHECK(resolve_rows(&b, &e, h) && b == h && e == h, "(h, h) is refused or changed: (%u, %u)", b, e);
    b = 0, e = h + 1;
    CHECK(!resolve_rows(&b, &e, h), "(0, h + 1) is accepted");
    b = 5, e = 4;
    CHECK(!resolve_rows(&b, &e, h), "(5, 4) is accepted");
    b = 4, e = 4;
    CHECK(resolve_rows(&b, &e, h) && b == 4 && e == 4, "the empty window (4, 4) became (%u, %u)", b, e);
    b = 3, e = h;
    CHECK(resolve_rows(&b, &e, h) && b == 3 && e == h, "(3, h) became (%u, %u)", b, e);
    b = 0, e = 0;
    CHECK(resolve_rows(&b, &e, 1) && b == 0 && e == 1, "(0, 0) of one row became (%u, %u)", b, e);
    b = 1, e = 1;
    CHECK(resolve_rows(&b, &e, 1) && b == 1 && e == 1, "(1, 1) of one row became (%u, %u)", b, e);
    b = 0, e = 0xffffffffu;
    CHECK(!resolve_rows(&b, &e, 0xfffffffeu), "(0, 2^32 - 1) of 2^32 - 2 rows is accepted");
}

}  // namespace

int main() {
    check_plane_status();
    check_byte_ranges();
    check_texel_count();
    check_rows();
    if (g_failures) {
        std::printf("plane_check: %d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("plane_check ok\n");
    return 0;
}
