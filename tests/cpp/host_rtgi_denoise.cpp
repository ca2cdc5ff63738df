// Frames of the filter for the RTGI ray planes through the C++ host façade (include/sah_host.hpp): RtgiDenoiser, one "RTGI denoise" pass
// and one depth copy per frame.  The frames' extents, jitters, ray, irradiance, depth, normal and motion-vector planes come from a file
// written by tests/test_rtgi_denoise_gpu.py; each frame's view block (as the façade's SceneView formed it) and its two denoised planes go
// back.  A frame of another extent makes the denoiser re-create its textures and start without a history.
//
//   host_rtgi_denoise <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_rtgi_denoise in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[2];  // frames, passes
    if (fread(hdr, 4, 2, in) != 2 || hdr[0] > 64) return 2;
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    RtgiDenoiser denoiser(alloc);
    const RtgiDenoiseSettings& s = denoiser.settings;  // the header's defaults
    if (s.passes != 3 || s.max_history != 32.f || s.min_history != 4.f || s.luminance_sigma != 4.f || s.luminance_floor != 1e-6f || s.normal_squarings != 5) return 1;
    denoiser.settings.passes = hdr[1];
    SceneView view;
    view.set_position({-7.f, 1.f, 0.f});
    view.rotate(0.1f, 1.2f);
    {  // the RTGI's denoise is opt-in, and without the motion vectors it is refused when the pass is recorded
        RayTracedGlobalIllumination rtgi(backend);
        if (rtgi.denoise || rtgi.denoise_motion_vectors || rtgi.get_denoised_ray_texture()) return 1;  // the defaults stay
        rtgi.denoise = true;
        RenderScene scene;
        RenderGraph graph{backend};
        bool refused = false;
        try {
            rtgi.post_render(graph, view, scene, GBuffer{}, nullptr);
        } catch (const std::logic_error&) {
            refused = true;
        }
        if (!refused) { fprintf(stderr, "RTGI without motion vectors recorded a denoised pass\n"); return 1; }
        rtgi.reset_denoise_history();  // (no denoiser yet: nothing to do)
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    for (uint32_t frame = 0; frame < hdr[0]; frame++) {
        uint32_t extent[2];
        float jitter[2];
        if (fread(extent, 4, 2, in) != 2 || fread(jitter, 4, 2, in) != 2 || !extent[0] || !extent[1] || extent[0] > 4096 || extent[1] > 4096) return 2;
        const uint32_t W = extent[0], H = extent[1];
        std::vector<unsigned char> rb((size_t)W * H * 8), ri((size_t)W * H * 8), d((size_t)W * H * 4), n((size_t)W * H * 8), m((size_t)W * H * 4);
        if (fread(rb.data(), 1, rb.size(), in) != rb.size() || fread(ri.data(), 1, ri.size(), in) != ri.size() || fread(d.data(), 1, d.size(), in) != d.size() ||
            fread(n.data(), 1, n.size(), in) != n.size() || fread(m.data(), 1, m.size(), in) != m.size())
            return 2;
        GBuffer gbuffer;
        gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
        gbuffer.normals = alloc.create_texture("gbuffer_normals", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        TextureHandle rays = alloc.create_texture("rtgi_params", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        TextureHandle irradiance = alloc.create_texture("rtgi_irradiance", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        TextureHandle motion = alloc.create_texture("motion_vectors", SAH_FORMAT_R16G16_SFLOAT, W, H);
        TextureHandle out_rays = alloc.create_texture("rtgi_params_denoised", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        TextureHandle out_irradiance = alloc.create_texture("rtgi_irradiance_denoised", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        alloc.upload(rays, rb.data(), W * 8);
        alloc.upload(irradiance, ri.data(), W * 8);
        alloc.upload(gbuffer.depth, d.data(), W * 4);
        alloc.upload(gbuffer.normals, n.data(), W * 8);
        alloc.upload(motion, m.data(), W * 4);
        view.set_render_resolution(W, H);
        view.set_perspective_projection(75.f, (float)W / (float)H, 0.05f);
        view.set_jitter(jitter[0], jitter[1]);
        view.update_transforms();
        RenderGraph graph{backend};
        denoiser.denoise(graph, view, rays, irradiance, gbuffer.depth, gbuffer.normals, motion, out_rays, out_irradiance);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty()) return 1;
        alloc.download(out_rays, rb.data(), W * 8);
        alloc.download(out_irradiance, ri.data(), W * 8);
        fwrite(&view.get_gpu_data(), sizeof(sah_view_data), 1, out);
        fwrite(rb.data(), 1, rb.size(), out);
        fwrite(ri.data(), 1, ri.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
