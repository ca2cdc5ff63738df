// One LPV frame through the C++ host façade (include/sah_host.hpp) with r.GI.LPV.GvBuildMode = DepthBuffers and use_gv on: the RSM GV
// injection after the VPL passes, the scene GV injection and the GV-occluded propagation in post_render.  Inputs (a G-buffer's depth and
// normals, the three injected colour volumes) come from tests/test_lpv_gv_facade_gpu.py; the GV and the propagated A volumes go back.
//
//   host_lpv_gv <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_lpv_gv in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[3];
    if (fread(hdr, 4, 3, in) != 3) return 2;
    const uint32_t W = hdr[0], H = hdr[1], steps = hdr[2];
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    GBuffer gbuffer;
    gbuffer.normals = alloc.create_texture("gbuffer_normals", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
    auto up = [&](TextureHandle t, uint32_t bpp) {
        std::vector<unsigned char> blob((size_t)t->desc.width * t->desc.height * t->desc.depth * bpp);
        if (fread(blob.data(), 1, blob.size(), in) != blob.size()) { fprintf(stderr, "short read\n"); exit(2); }
        alloc.upload(t, blob.data(), t->desc.width * bpp);
    };
    up(gbuffer.normals, 8);
    up(gbuffer.depth, 4);
    RenderScene scene;
    SceneView view;  // start-up camera of the reference: scene_renderer.cpp:53-54,105-116
    view.rotate(0.f, 90.f * 3.14159265358979f / 180.f);
    view.set_position({-7.f, 1.f, 0.f});
    view.set_render_resolution(W, H);
    view.set_perspective_projection(75.f, (float)W / (float)H, 0.05f);
    view.update_transforms();
    LightPropagationVolume lpv(backend, 4, steps);
    lpv.gv_build_mode = LightPropagationVolume::GvBuildMode::DepthBuffers;
    lpv.use_gv = true;
    lpv.update_cascade_transforms(view, scene.sun);
    RenderGraph graph{backend};
    lpv.pre_render(graph, view, scene, nullptr);  // clears the colour volumes and the GV
    graph.finish();
    if (!graph.get_errors().empty()) { fprintf(stderr, "pass failed: %s\n", graph.get_errors()[0].c_str()); return 1; }
    for (int c = 0; c < 3; c++) up(lpv.get_volume(c), 8);  // stands in for the RSM render + VPL injection
    RenderGraph gv_frame{backend};
    IGlobalIlluminator* gi = &lpv;
    gi->post_render(gv_frame, view, scene, gbuffer, nullptr);
    gv_frame.finish();
    for (const auto& e : gv_frame.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
    if (!gv_frame.get_errors().empty()) return 1;
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    fwrite(&view.get_gpu_data(), sizeof(sah_view_data), 1, out);
    fwrite(lpv.get_cascade_matrices(), sizeof(sah_lpv_cascade_matrices), 4, out);
    std::vector<unsigned char> v((size_t)128 * 32 * 32 * 8);
    alloc.download(lpv.get_geometry_volume(), v.data(), 128 * 8);
    fwrite(v.data(), 1, v.size(), out);
    for (int c = 0; c < 3; c++) {
        alloc.download(lpv.get_volume(c, steps & 1), v.data(), 128 * 8);
        fwrite(v.data(), 1, v.size(), out);
    }
    fclose(out);
    return 0;
}
