// The Hi-Z pyramid of a depth plane through the C++ host façade (include/sah_host.hpp): DepthCullingPhase::set_render_resolution and
// build_hi_z, twice (the second frame finds the counter as the first left it).  The depth plane comes from a file written by
// tests/test_mip_chain_facade_gpu.py; the level count and every level's texels go back.
//
//   host_hi_z <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_hi_z in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[2];  // W, H
    if (fread(hdr, 4, 2, in) != 2) return 2;
    const uint32_t W = hdr[0], H = hdr[1];
    std::vector<unsigned char> depth((size_t)W * H * 4);
    if (fread(depth.data(), 1, depth.size(), in) != depth.size()) return 2;
    fclose(in);
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    TextureHandle depth_buffer = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
    alloc.upload(depth_buffer, depth.data(), W * 4);
    DepthCullingPhase phase(alloc);
    const uint32_t resolution[2] = {W, H};
    phase.set_render_resolution(resolution);
    for (int frame = 0; frame < 2; frame++) {
        RenderGraph graph{backend};
        phase.build_hi_z(graph, depth_buffer);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty()) return 1;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    const uint32_t n = (uint32_t)phase.get_hi_z_levels().size();
    fwrite(&n, 4, 1, out);
    std::vector<unsigned char> buf;
    for (TextureHandle level : phase.get_hi_z_levels()) {
        const uint32_t extent[2] = {level->desc.width, level->desc.height};
        fwrite(extent, 4, 2, out);
        buf.resize((size_t)extent[0] * extent[1] * 4);
        alloc.download(level, buf.data(), extent[0] * 4);
        fwrite(buf.data(), 1, buf.size(), out);
    }
    fclose(out);
    return 0;
}
