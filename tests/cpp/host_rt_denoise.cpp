// Frames of the filter for the ray-traced masks through the C++ host façade (include/sah_host.hpp): RayTracedDenoiser, one "Ray-traced
// denoise" pass and one depth copy per frame.  The frames' extents, jitters, sample, depth, normal and motion-vector planes come from a file
// written by tests/test_rt_denoise_gpu.py; each frame's view block (as the façade's SceneView formed it) and denoised plane go back.  A
// frame of another extent makes the denoiser re-create its textures and start without a history.
//
//   host_rt_denoise <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_rt_denoise in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[2];  // frames, passes
    if (fread(hdr, 4, 2, in) != 2 || hdr[0] > 64) return 2;
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    RayTracedDenoiser denoiser(alloc);
    if (denoiser.settings.passes != 3 || denoiser.settings.max_history != 32.f) return 1;  // the header's defaults
    denoiser.settings.passes = hdr[1];
    SceneView view;
    view.set_position({-7.f, 1.f, 0.f});
    view.rotate(0.1f, 1.2f);
    {  // the AO phase's denoise is opt-in, and a phase without an allocator (or without the motion vectors) refuses it when the pass is recorded
        AmbientOcclusionPhase bare;
        if (bare.denoise || bare.technique != AoTechnique::RTAO) return 1;  // the defaults stay
        bare.denoise = true;
        RenderScene scene;
        NoiseTexture no_noise;
        RenderGraph graph{backend};
        bool refused = false;
        try {
            bare.generate_ao(graph, view, scene, no_noise, nullptr, nullptr, nullptr);
        } catch (const std::logic_error&) {
            refused = true;
        }
        if (!refused) { fprintf(stderr, "a phase without an allocator recorded a denoised pass\n"); return 1; }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    for (uint32_t frame = 0; frame < hdr[0]; frame++) {
        uint32_t extent[2];
        float jitter[2];
        if (fread(extent, 4, 2, in) != 2 || fread(jitter, 4, 2, in) != 2 || !extent[0] || !extent[1] || extent[0] > 4096 || extent[1] > 4096) return 2;
        const uint32_t W = extent[0], H = extent[1];
        std::vector<unsigned char> s((size_t)W * H * 4), d((size_t)W * H * 4), n((size_t)W * H * 8), m((size_t)W * H * 4);
        if (fread(s.data(), 1, s.size(), in) != s.size() || fread(d.data(), 1, d.size(), in) != d.size() || fread(n.data(), 1, n.size(), in) != n.size() ||
            fread(m.data(), 1, m.size(), in) != m.size())
            return 2;
        GBuffer gbuffer;
        gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
        gbuffer.normals = alloc.create_texture("gbuffer_normals", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        TextureHandle noisy = alloc.create_texture("ao_raw", SAH_FORMAT_R32_SFLOAT, W, H);
        TextureHandle motion = alloc.create_texture("motion_vectors", SAH_FORMAT_R16G16_SFLOAT, W, H);
        TextureHandle ao = alloc.create_texture("ao", SAH_FORMAT_R32_SFLOAT, W, H);
        alloc.upload(noisy, s.data(), W * 4);
        alloc.upload(gbuffer.depth, d.data(), W * 4);
        alloc.upload(gbuffer.normals, n.data(), W * 8);
        alloc.upload(motion, m.data(), W * 4);
        view.set_render_resolution(W, H);
        view.set_perspective_projection(75.f, (float)W / (float)H, 0.05f);
        view.set_jitter(jitter[0], jitter[1]);
        view.update_transforms();
        RenderGraph graph{backend};
        denoiser.denoise(graph, view, noisy, gbuffer.depth, gbuffer.normals, motion, ao);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty()) return 1;
        alloc.download(ao, s.data(), W * 4);
        fwrite(&view.get_gpu_data(), sizeof(sah_view_data), 1, out);
        fwrite(s.data(), 1, s.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
