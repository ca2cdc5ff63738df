// Frames of temporal anti-aliasing through the C++ host façade (include/sah_host.hpp): TemporalAntiAliasing behind the IUpscaler seam, the
// jitter it hands out set on the view, one "Temporal AA" pass per frame.  The frames' lit, depth and motion-vector planes come from a file
// written by tests/test_taa_gpu.py; each frame's jitter and resolved image go back.
//
//   host_taa <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_taa in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[4];  // W, H, frames, hdr weights
    float blend;
    if (fread(hdr, 4, 4, in) != 4 || fread(&blend, 4, 1, in) != 1 || hdr[2] > 64) return 2;
    const uint32_t W = hdr[0], H = hdr[1], frames = hdr[2];
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    GBuffer gbuffer;
    gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
    TextureHandle lit = alloc.create_texture("lit_scene", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    TextureHandle antialiased = alloc.create_texture("antialiased_scene", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    TextureHandle motion = alloc.create_texture("motion_vectors", SAH_FORMAT_R16G16_SFLOAT, W, H);
    TemporalAntiAliasing taa(alloc);
    taa.blend = blend;
    taa.hdr_weights = hdr[3] != 0;
    const uint32_t resolution[2] = {W, H};
    taa.initialize(resolution, 0);
    if (taa.get_optimal_render_resolution()[0] != W || taa.get_optimal_render_resolution()[1] != H) return 1;
    IUpscaler& upscaler = taa;
    SceneView view;
    view.set_render_resolution(W, H);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    std::vector<unsigned char> l((size_t)W * H * 8), d((size_t)W * H * 4), m((size_t)W * H * 4);
    for (uint32_t frame = 0; frame < frames; frame++) {
        if (fread(l.data(), 1, l.size(), in) != l.size() || fread(d.data(), 1, d.size(), in) != d.size() || fread(m.data(), 1, m.size(), in) != m.size()) return 2;
        alloc.upload(lit, l.data(), W * 8);
        alloc.upload(gbuffer.depth, d.data(), W * 4);
        alloc.upload(motion, m.data(), W * 4);
        const auto jitter = upscaler.get_jitter();  // SceneRenderer::update_jitter, scene_renderer.cpp:684-691
        view.set_jitter(jitter[0], jitter[1]);
        view.update_transforms();
        upscaler.set_constants(view, resolution);
        RenderGraph graph{backend};
        upscaler.evaluate(graph, view, gbuffer, lit, antialiased, motion);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty()) return 1;
        alloc.download(antialiased, l.data(), W * 8);
        fwrite(jitter.data(), 4, 2, out);
        fwrite(l.data(), 1, l.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
