// Two frames of the VRSAA passes through the C++ host façade (include/sah_host.hpp): generate_shading_rate_image from the last frame's
// contrast image, then measure_aliasing on this frame's colour and depth, in the reference's order.  Colour and depth come from a file
// written by tests/test_vrsaa_facade_gpu.py; the shading-rate images of both frames and the contrast image go back.
//
//   host_vrsaa <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_vrsaa in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[5];  // W, H, texel size x, y, number of rates
    if (fread(hdr, 4, 5, in) != 5 || hdr[4] > 8) return 2;
    const uint32_t W = hdr[0], H = hdr[1];
    std::vector<std::array<uint32_t, 2>> rates(hdr[4]);
    if (hdr[4] && fread(rates.data(), 8, hdr[4], in) != hdr[4]) return 2;
    std::vector<unsigned char> color((size_t)W * H * 4), depth((size_t)W * H * 4);
    if (fread(color.data(), 1, color.size(), in) != color.size() || fread(depth.data(), 1, depth.size(), in) != depth.size()) return 2;
    fclose(in);
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    GBuffer gbuffer;
    gbuffer.color = alloc.create_texture("gbuffer_color", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
    gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
    alloc.upload(gbuffer.color, color.data(), W * 4);
    alloc.upload(gbuffer.depth, depth.data(), W * 4);
    VRSAA vrsaa(alloc);
    vrsaa.set_max_shading_rate_texel_size(hdr[2], hdr[3]);
    vrsaa.set_shading_rates(rates);
    const uint32_t resolution[2] = {W, H};
    vrsaa.init(resolution);
    const uint32_t SW = vrsaa.get_shading_rate_image()->desc.width, SH = vrsaa.get_shading_rate_image()->desc.height;
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    const uint32_t extent[2] = {SW, SH};
    fwrite(extent, 4, 2, out);
    std::vector<unsigned char> buf;
    for (int frame = 0; frame < 2; frame++) {
        RenderGraph graph{backend};
        vrsaa.generate_shading_rate_image(graph);
        vrsaa.measure_aliasing(graph, gbuffer.color, gbuffer.depth);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty()) return 1;
        buf.resize((size_t)SW * SH);
        alloc.download(vrsaa.get_shading_rate_image(), buf.data(), SW);
        fwrite(buf.data(), 1, buf.size(), out);
    }
    buf.resize((size_t)W * H * 4);
    alloc.download(vrsaa.get_contrast_image(), buf.data(), W * 4);
    fwrite(buf.data(), 1, buf.size(), out);
    fclose(out);
    return 0;
}
