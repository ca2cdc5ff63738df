// Frames of screen-space ambient occlusion through the C++ host façade (include/sah_host.hpp): AmbientOcclusionPhase with
// AoTechnique::ScreenSpace, one "Screen-space ambient occlusion" pass per frame through the scene overload of generate_ao — no noise
// texture, no acceleration structure.  The frames' extents, jitters, depth and normal planes come from a file written by
// tests/test_ssao_gpu.py; each frame's view block (as the façade's SceneView formed it) and AO plane go back.  A frame of another extent
// makes the phase re-create its scratch texture.
//
//   host_ssao <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_ssao in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[2];  // frames, blur passes
    float radius;
    if (fread(hdr, 4, 2, in) != 2 || fread(&radius, 4, 1, in) != 1 || hdr[0] > 64) return 2;
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    AmbientOcclusionPhase ao_phase(alloc);
    if (ao_phase.technique != AoTechnique::RTAO) return 1;  // the default stays
    ao_phase.technique = AoTechnique::ScreenSpace;
    ao_phase.ao_radius = radius;
    ao_phase.screen_space.blur_passes = hdr[1];
    RenderScene scene;      // empty: nothing is built, and nothing needs to be
    NoiseTexture no_noise;  // not read
    SceneView view;
    view.set_position({-7.f, 1.f, 0.f});
    view.rotate(0.1f, 1.2f);
    {  // a phase without an allocator has nowhere to keep the raw plane: with a blur it refuses when the pass is recorded
        AmbientOcclusionPhase bare;
        bare.technique = AoTechnique::ScreenSpace;
        RenderGraph graph{backend};
        bool refused = false;
        try {
            bare.generate_ao(graph, view, scene, no_noise, nullptr, nullptr, nullptr);
        } catch (const std::logic_error&) {
            refused = true;
        }
        if (!refused) { fprintf(stderr, "a phase without an allocator recorded a blurred pass\n"); return 1; }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    for (uint32_t frame = 0; frame < hdr[0]; frame++) {
        uint32_t extent[2];
        float jitter[2];
        if (fread(extent, 4, 2, in) != 2 || fread(jitter, 4, 2, in) != 2 || !extent[0] || !extent[1] || extent[0] > 4096 || extent[1] > 4096) return 2;
        const uint32_t W = extent[0], H = extent[1];
        std::vector<unsigned char> d((size_t)W * H * 4), n((size_t)W * H * 8);
        if (fread(d.data(), 1, d.size(), in) != d.size() || fread(n.data(), 1, n.size(), in) != n.size()) return 2;
        GBuffer gbuffer;
        gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
        gbuffer.normals = alloc.create_texture("gbuffer_normals", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        TextureHandle ao = alloc.create_texture("ao", SAH_FORMAT_R32_SFLOAT, W, H);
        alloc.upload(gbuffer.depth, d.data(), W * 4);
        alloc.upload(gbuffer.normals, n.data(), W * 8);
        view.set_render_resolution(W, H);
        view.set_perspective_projection(75.f, (float)W / (float)H, 0.05f);
        view.set_jitter(jitter[0], jitter[1]);
        view.update_transforms();
        RenderGraph graph{backend};
        ao_phase.generate_ao(graph, view, scene, no_noise, gbuffer.normals, gbuffer.depth, ao);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty()) return 1;
        alloc.download(ao, d.data(), W * 4);
        fwrite(&view.get_gpu_data(), sizeof(sah_view_data), 1, out);
        fwrite(d.data(), 1, d.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
