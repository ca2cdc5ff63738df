// Frames of temporal upscaling through the C++ host façade (include/sah_host.hpp): TemporalUpscaling behind the IUpscaler seam, the render
// resolution and the jitter it hands out, one "Temporal upscale" pass per frame.  The frames' lit, depth and motion-vector planes (at the
// render resolution the façade asks for) come from a file written by tests/test_taa_upscale_gpu.py; the render resolution, the number of
// jitter phases, and each frame's jitter and resolved image go back.
//
//   host_taa_upscale <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_taa_upscale in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[4];  // W, H (output), frames, hdr weights
    float cfg[3];     // blend, min_confidence, scale
    if (fread(hdr, 4, 4, in) != 4 || fread(cfg, 4, 3, in) != 3 || hdr[2] > 64) return 2;
    const uint32_t W = hdr[0], H = hdr[1], frames = hdr[2];
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    TemporalUpscaling upscaling(alloc, cfg[2]);
    upscaling.blend = cfg[0];
    upscaling.min_confidence = cfg[1];
    upscaling.hdr_weights = hdr[3] != 0;
    const uint32_t output[2] = {W, H};
    upscaling.initialize(output, 0);
    IUpscaler& upscaler = upscaling;
    const auto render = upscaler.get_optimal_render_resolution();
    const uint32_t w = render[0], h = render[1], resolution[2] = {w, h};
    GBuffer gbuffer;
    gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, w, h);
    TextureHandle lit = alloc.create_texture("lit_scene", SAH_FORMAT_R16G16B16A16_SFLOAT, w, h);
    TextureHandle motion = alloc.create_texture("motion_vectors", SAH_FORMAT_R16G16_SFLOAT, w, h);
    TextureHandle upscaled = alloc.create_texture("antialiased_scene", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    SceneView view;
    view.set_render_resolution(w, h);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    const uint32_t facts[3] = {w, h, upscaling.get_jitter_phase_count()};
    fwrite(facts, 4, 3, out);
    std::vector<unsigned char> l((size_t)w * h * 8), d((size_t)w * h * 4), m((size_t)w * h * 4), o((size_t)W * H * 8);
    for (uint32_t frame = 0; frame < frames; frame++) {
        if (fread(l.data(), 1, l.size(), in) != l.size() || fread(d.data(), 1, d.size(), in) != d.size() || fread(m.data(), 1, m.size(), in) != m.size()) return 2;
        alloc.upload(lit, l.data(), w * 8);
        alloc.upload(gbuffer.depth, d.data(), w * 4);
        alloc.upload(motion, m.data(), w * 4);
        const auto jitter = upscaler.get_jitter();  // SceneRenderer::update_jitter, scene_renderer.cpp:684-691
        view.set_jitter(jitter[0], jitter[1]);
        view.update_transforms();
        upscaler.set_constants(view, resolution);
        RenderGraph graph{backend};
        upscaler.evaluate(graph, view, gbuffer, lit, upscaled, motion);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty()) return 1;
        alloc.download(upscaled, o.data(), W * 8);
        fwrite(jitter.data(), 4, 2, out);
        fwrite(o.data(), 1, o.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
