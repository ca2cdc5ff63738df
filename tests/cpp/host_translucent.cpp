// TranslucencyPhase through the C++ host façade (include/sah_host.hpp): GbufferPhase on the opaque half of a scene, LightingPhase (sun off,
// LPV, sky) into two lit images, and TranslucencyPhase after the second — so that the first is the frame the façade writes without the
// phase.  The mesh (one set of vertex, index and material arrays, two primitive lists: opaque and translucent, the latter back to front)
// and the frame's side inputs come from a file written by tests/test_translucent_facade_gpu.py; the uniform blocks this program builds go
// back with the images, so that the test can make the direct calls on the very same blocks.  A third lit image is what the phase gives
// when it is recorded with no Lighting pass before it in a graph of its own: untouched, and an error logged.
//
//   host_translucent <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

static std::vector<unsigned char> read_blob(FILE* f, size_t n) {
    std::vector<unsigned char> v(n);
    if (n && fread(v.data(), 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
static void* to_device(FILE* f, size_t n) {
    if (n == 0) return nullptr;
    auto v = read_blob(f, n);
    void* p = nullptr;
    if (hipMalloc(&p, n) != hipSuccess || hipMemcpy(p, v.data(), n, hipMemcpyHostToDevice) != hipSuccess) exit(3);
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_translucent in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[8];  // W, H, LPV steps, vertices, indices, materials, opaque primitives, translucent primitives
    if (fread(hdr, 4, 8, in) != 8) return 2;
    const uint32_t W = hdr[0], H = hdr[1], lpv_steps = hdr[2];

    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    RenderScene scene;
    sah_scene_geometry& g = scene.geometry;
    g.num_vertices = hdr[3];
    g.num_indices = hdr[4];
    g.num_materials = hdr[5];
    g.vertex_positions = (const float*)to_device(in, (size_t)hdr[3] * 12);
    g.vertex_data = (const sah_vertex_data*)to_device(in, (size_t)hdr[3] * sizeof(sah_vertex_data));
    g.indices = (const uint32_t*)to_device(in, (size_t)hdr[4] * 4);
    g.materials = (const sah_material*)to_device(in, (size_t)hdr[5] * sizeof(sah_material));
    sah_scene_geometry translucent = g;  // the same streams, the other primitive list
    g.num_primitives = hdr[6];
    g.primitives = (const sah_primitive*)to_device(in, (size_t)hdr[6] * sizeof(sah_primitive));
    translucent.num_primitives = hdr[7];
    translucent.primitives = (const sah_primitive*)to_device(in, (size_t)hdr[7] * sizeof(sah_primitive));

    GBuffer gbuffer;
    gbuffer.color = alloc.create_texture("gbuffer_color", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
    gbuffer.normals = alloc.create_texture("gbuffer_normals", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    gbuffer.data = alloc.create_texture("gbuffer_data", SAH_FORMAT_R8G8B8A8_UNORM, W, H);
    gbuffer.emission = alloc.create_texture("gbuffer_emission", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
    gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
    TextureHandle ao = alloc.create_texture("ao", SAH_FORMAT_R32_SFLOAT, W, H);
    TextureHandle lit[3];
    for (int i = 0; i < 3; i++) lit[i] = alloc.create_texture("lit_scene", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    scene.sky.transmittance_lut = alloc.create_texture("Transmittance LUT", SAH_FORMAT_R16G16B16A16_SFLOAT, 256, 64);
    scene.sky.sky_view_lut = alloc.create_texture("Sky view LUT", SAH_FORMAT_R16G16B16A16_SFLOAT, 200, 200);
    scene.sun.set_shadow_mode(SunShadowMode::Off);

    auto up = [&](TextureHandle t, uint32_t bpp) {
        auto blob = read_blob(in, (size_t)t->desc.width * t->desc.height * t->desc.depth * bpp);
        alloc.upload(t, blob.data(), t->desc.width * bpp);
    };
    up(ao, 4);
    up(scene.sky.transmittance_lut, 8); up(scene.sky.sky_view_lut, 8);
    up(lit[2], 8);  // a pattern that must survive the phase recorded without a Lighting pass

    SceneView view;  // start-up camera of the reference: scene_renderer.cpp:53-54,105-116
    view.rotate(0.f, 90.f * 3.14159265358979f / 180.f);
    view.set_position({-7.f, 1.f, 0.f});
    view.set_render_resolution(W, H);
    view.set_perspective_projection(75.f, (float)W / (float)H, 0.05f);
    view.update_transforms();

    LightPropagationVolume lpv(backend, 4, lpv_steps);
    lpv.update_cascade_transforms(view, scene.sun);
    for (int c = 0; c < 3; c++) up(lpv.get_volume(c), 8);  // stands in for RSM/VPL injection
    fclose(in);

    RenderGraph graph{backend};
    NoiseTexture stbn_3d_unitvec, stbn_2d_scalar;
    IGlobalIlluminator* gi = &lpv;
    GbufferPhase gbuffer_phase;
    gbuffer_phase.render(graph, scene, gbuffer, view);  // scene.geometry: the opaque half
    gi->post_render(graph, view, scene, gbuffer, stbn_3d_unitvec.get_layer(0));
    LightingPhase lighting;
    lighting.set_scene(scene);
    TranslucencyPhase translucency;
    // 0: the frame as it is without the phase
    lighting.render(graph, view, gbuffer, lit[0], ao, gi, std::nullopt, stbn_3d_unitvec, stbn_2d_scalar.get_layer(0));
    // 1: Lighting, then the translucent primitives blended into its lit image
    lighting.render(graph, view, gbuffer, lit[1], ao, gi, std::nullopt, stbn_3d_unitvec, stbn_2d_scalar.get_layer(0));
    translucency.render(graph, translucent);
    graph.finish();
    for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
    if (!graph.get_errors().empty()) return 1;
    // 2: no Lighting pass in the graph: refused, logged, nothing written
    RenderGraph alone{backend};
    translucency.render(alone, translucent);
    alone.finish();
    if (alone.get_errors().size() != 1) { fprintf(stderr, "the phase without a Lighting pass logged %zu errors, not 1\n", alone.get_errors().size()); return 1; }

    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    fwrite(&view.get_gpu_data(), sizeof(sah_view_data), 1, out);
    fwrite(&scene.sun.get_constants(), sizeof(sah_sun_light_constants), 1, out);
    fwrite(lpv.get_cascade_matrices(), sizeof(sah_lpv_cascade_matrices), 4, out);
    for (int c = 0; c < 3; c++) {  // propagated LPV (A volumes)
        std::vector<unsigned char> v((size_t)128 * 32 * 32 * 8);
        alloc.download(lpv.get_volume(c), v.data(), 128 * 8);
        fwrite(v.data(), 1, v.size(), out);
    }
    const struct { TextureHandle t; uint32_t bpp; } planes[8] = {{gbuffer.color, 4}, {gbuffer.normals, 8}, {gbuffer.data, 4}, {gbuffer.emission, 4}, {gbuffer.depth, 4},
                                                                   {lit[0], 8}, {lit[1], 8}, {lit[2], 8}};
    std::vector<unsigned char> buf;
    for (const auto& p : planes) {
        buf.resize((size_t)W * H * p.bpp);
        alloc.download(p.t, buf.data(), W * p.bpp);
        fwrite(buf.data(), 1, buf.size(), out);
    }
    fclose(out);
    return 0;
}
