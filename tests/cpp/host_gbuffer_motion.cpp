// GbufferPhase and MotionVectorsPhase (needs_motion_vectors on) through the C++ host façade (include/sah_host.hpp), for a camera that
// moved and turned between the last frame and this one.  The mesh comes from a file written by tests/test_gbuffer_motion_facade_gpu.py;
// the view block built here and the six planes go back.  The third argument is MotionVectorsPhase::share_gbuffer_setup: with 1 the
// G-buffer phase records the one fused pass (sah_gbuffer_motion_render) and the motion phase nothing, with 0 each records its own.
// Prints the number of passes the graph recorded.
//
//   host_gbuffer_motion <in.bin> <out.bin> <0|1>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

static void* to_device(FILE* f, size_t n) {
    std::vector<unsigned char> v(n);
    void* p = nullptr;
    if (n == 0) return nullptr;
    if (fread(v.data(), 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    if (hipMalloc(&p, n) != hipSuccess || hipMemcpy(p, v.data(), n, hipMemcpyHostToDevice) != hipSuccess) exit(3);
    return p;
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: host_gbuffer_motion in.bin out.bin 0|1\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[6];  // W, H, vertices, indices, primitives, materials
    if (fread(hdr, 4, 6, in) != 6) return 2;
    const uint32_t W = hdr[0], H = hdr[1];
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    RenderScene scene;
    scene.geometry.num_vertices = hdr[2];
    scene.geometry.num_indices = hdr[3];
    scene.geometry.num_primitives = hdr[4];
    scene.geometry.num_materials = hdr[5];
    scene.geometry.vertex_positions = (const float*)to_device(in, (size_t)hdr[2] * 12);
    scene.geometry.vertex_data = (const sah_vertex_data*)to_device(in, (size_t)hdr[2] * sizeof(sah_vertex_data));
    scene.geometry.indices = (const uint32_t*)to_device(in, (size_t)hdr[3] * 4);
    scene.geometry.primitives = (const sah_primitive*)to_device(in, (size_t)hdr[4] * sizeof(sah_primitive));
    scene.geometry.materials = (const sah_material*)to_device(in, (size_t)hdr[5] * sizeof(sah_material));
    fclose(in);
    SceneView view;
    view.rotate(0.f, 90.f * 3.14159265358979f / 180.f);
    view.set_position({-7.f, 1.f, 0.f});
    view.set_render_resolution(W, H);
    view.set_perspective_projection(75.f, (float)W / (float)H, 0.05f);
    view.update_transforms();  // the last frame
    view.rotate(0.02f, 0.03f);
    view.set_position({-7.3f, 1.1f, 0.2f});
    view.update_transforms();  // this frame
    GBuffer gbuffer;
    gbuffer.color = alloc.create_texture("gbuffer_color", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
    gbuffer.normals = alloc.create_texture("gbuffer_normals", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    gbuffer.data = alloc.create_texture("gbuffer_data", SAH_FORMAT_R8G8B8A8_UNORM, W, H);
    gbuffer.emission = alloc.create_texture("gbuffer_emission", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
    gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
    MotionVectorsPhase motion_vectors_phase(alloc);
    motion_vectors_phase.needs_motion_vectors = true;
    motion_vectors_phase.share_gbuffer_setup = argv[3][0] == '1';
    const uint32_t resolution[2] = {W, H};
    motion_vectors_phase.set_render_resolution(resolution, resolution);
    RenderGraph graph{backend};
    GbufferPhase gbuffer_phase;
    gbuffer_phase.render(graph, scene, gbuffer, view, &motion_vectors_phase);
    motion_vectors_phase.render(graph, scene, view, gbuffer.depth);
    graph.finish();
    for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
    if (!graph.get_errors().empty()) return 1;
    printf("passes %u\n", graph.get_num_passes());
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    fwrite(&view.get_gpu_data(), sizeof(sah_view_data), 1, out);
    const struct { TextureHandle t; uint32_t bpp; } planes[6] = {{gbuffer.color, 4}, {gbuffer.normals, 8}, {gbuffer.data, 4}, {gbuffer.emission, 4},
                                                                   {gbuffer.depth, 4}, {motion_vectors_phase.get_motion_vectors(), 4}};
    std::vector<unsigned char> buf;
    for (const auto& p : planes) {
        buf.resize((size_t)W * H * p.bpp);
        alloc.download(p.t, buf.data(), W * p.bpp);
        fwrite(buf.data(), 1, buf.size(), out);
    }
    fclose(out);
    return 0;
}
