// Two traced frames through the C++ host façade (include/sah_host.hpp) with one primitive moved in between: RaytracingScene::finalize
// records "Build TLAS" for the first frame and, for the second, "Refit TLAS" (update_primitive: sah_rt_refit) or "Build TLAS" again
// (add_primitive).  Ray results do not depend on which (include/sah_rt_refit.h), so the hashes this prints are the same in both modes.
// The mesh comes from a file written by tests/test_rt_refit_facade_gpu.py.
//
//   host_rt_refit <in.bin> refit|rebuild
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sah_host.hpp"

static std::vector<unsigned char> read_blob(FILE* f, size_t n) {
    std::vector<unsigned char> v(n);
    if (n && fread(v.data(), 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
static void* to_device(const std::vector<unsigned char>& v) {
    void* p = nullptr;
    if (v.empty()) return nullptr;
    if (hipMalloc(&p, v.size()) != hipSuccess || hipMemcpy(p, v.data(), v.size(), hipMemcpyHostToDevice) != hipSuccess) exit(3);
    return p;
}
static unsigned long long fnv1a(const std::vector<unsigned char>& v) {
    unsigned long long h = 0xcbf29ce484222325ull;
    for (unsigned char c : v) h = (h ^ c) * 0x100000001b3ull;
    return h;
}

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[2], "refit") && strcmp(argv[2], "rebuild"))) { fprintf(stderr, "usage: host_rt_refit in.bin refit|rebuild\n"); return 2; }
    const bool refit = !strcmp(argv[2], "refit");
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[7];  // W, H, vertices, indices, primitives, materials, the primitive that moves
    if (fread(hdr, 4, 7, in) != 7) return 2;
    const uint32_t W = hdr[0], H = hdr[1], moving = hdr[6];
    if (moving >= hdr[4]) return 2;

    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    RenderScene scene;
    scene.geometry.num_vertices = hdr[2];
    scene.geometry.num_indices = hdr[3];
    scene.geometry.num_primitives = hdr[4];
    scene.geometry.num_materials = hdr[5];
    scene.geometry.vertex_positions = (const float*)to_device(read_blob(in, (size_t)hdr[2] * 12));
    scene.geometry.vertex_data = (const sah_vertex_data*)to_device(read_blob(in, (size_t)hdr[2] * sizeof(sah_vertex_data)));
    scene.geometry.indices = (const uint32_t*)to_device(read_blob(in, (size_t)hdr[3] * 4));
    sah_primitive* primitives = (sah_primitive*)to_device(read_blob(in, (size_t)hdr[4] * sizeof(sah_primitive)));
    scene.geometry.primitives = primitives;
    scene.geometry.materials = (const sah_material*)to_device(read_blob(in, (size_t)hdr[5] * sizeof(sah_material)));
    NoiseTexture noise;
    {
        TextureHandle layer = alloc.create_texture("stbn_unitvec3_2Dx1D_128x128x64_0", SAH_FORMAT_R8G8B8A8_UNORM, 128, 128);
        const auto texels = read_blob(in, 128 * 128 * 4);
        alloc.upload(layer, texels.data(), 128 * 4);
        noise.layers.push_back(layer);
        noise.resolution[0] = noise.resolution[1] = 128;
        noise.num_layers = 1;
    }
    const auto new_model = read_blob(in, 64);  // the moving primitive's model matrix in the second frame
    fclose(in);

    SceneView view;
    view.rotate(0.f, 90.f * 3.14159265358979f / 180.f);
    view.set_position({-7.f, 1.f, 0.f});
    view.set_render_resolution(W, H);
    view.set_perspective_projection(75.f, (float)W / (float)H, 0.05f);
    view.update_transforms();

    GBuffer gbuffer;
    gbuffer.color = alloc.create_texture("gbuffer_color", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
    gbuffer.normals = alloc.create_texture("gbuffer_normals", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    gbuffer.data = alloc.create_texture("gbuffer_data", SAH_FORMAT_R8G8B8A8_UNORM, W, H);
    gbuffer.emission = alloc.create_texture("gbuffer_emission", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
    gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
    TextureHandle ao = alloc.create_texture("ao", SAH_FORMAT_R32_SFLOAT, W, H);
    scene.sun.shadow_mask = alloc.create_texture("sun shadow mask", SAH_FORMAT_R32_SFLOAT, W, H);
    scene.sun.get_constants().num_shadow_samples = 2.0f;
    TextureHandle lit_scene = alloc.create_texture("lit_scene", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);

    GbufferPhase gbuffer_phase;
    AmbientOcclusionPhase ao_phase;
    ao_phase.technique = AoTechnique::RTAO;
    RaytracingScene& rt = scene.get_raytracing_scene();
    for (uint32_t p = 0; p < scene.geometry.num_primitives; p++) rt.add_primitive(p);
    for (int frame = 0; frame < 2; frame++) {
        RenderGraph graph{backend};
        if (frame == 1) {  // the transform is uploaded, then the scene is told
            if (hipMemcpy(primitives[moving].model, new_model.data(), 64, hipMemcpyHostToDevice) != hipSuccess) return 3;
            if (refit) rt.update_primitive(moving);
            else rt.add_primitive(moving);
        }
        gbuffer_phase.render(graph, scene, gbuffer, view);
        rt.finalize(graph);
        const RaytracingScene::Commit want = frame == 0 || !refit ? RaytracingScene::Commit::Build : RaytracingScene::Commit::Refit;
        if (rt.last_commit() != want) { fprintf(stderr, "frame %d: finalize recorded the wrong pass\n", frame); return 1; }
        ao_phase.generate_ao(graph, view, scene, noise, gbuffer.normals, gbuffer.depth, ao);
        scene.sun.raytrace(graph, view, gbuffer, scene, lit_scene, noise);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty()) return 1;
        std::vector<unsigned char> a((size_t)W * H * 4), m((size_t)W * H * 4), d((size_t)W * H * 4);
        alloc.download(ao, a.data(), W * 4);
        alloc.download(scene.sun.shadow_mask, m.data(), W * 4);
        alloc.download(gbuffer.depth, d.data(), W * 4);
        printf("frame %d %s depth %016llx ao %016llx mask %016llx\n", frame, want == RaytracingScene::Commit::Refit ? "Refit TLAS" : "Build TLAS", fnv1a(d),
               fnv1a(a), fnv1a(m));
    }
    // a frame in which nothing moved records neither pass
    RenderGraph graph{backend};
    rt.finalize(graph);
    if (rt.last_commit() != RaytracingScene::Commit::None || graph.get_num_passes() != 0) { fprintf(stderr, "an idle finalize recorded a pass\n"); return 1; }
    return 0;
}
