// LPV mesh lights through the C++ host façade (include/sah_host.hpp): RenderScene::generate_emissive_point_clouds on a host mesh, then
// three frames of LightPropagationVolume — the sun chain with mesh_lights off, the sun chain with mesh_lights on, and the mesh-light
// injection alone onto cleared volumes.  The mesh (host arrays) comes from tests/test_lpv_mesh_lights_facade_gpu.py; the cascade
// matrices and bounds, the pass counts and the three frames' A volumes go back.
//
//   host_lpv_mesh_lights <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

template <class T> static std::vector<T> take(FILE* in, uint32_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
template <class T> static T* upload(const std::vector<T>& v) {
    T* d = nullptr;
    if (hipMalloc((void**)&d, v.size() * sizeof(T) + 16) != hipSuccess || hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) exit(3);
    return d;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_lpv_mesh_lights in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[6];  // vertices, indices, primitives, materials, seed, flags
    if (fread(hdr, 4, 6, in) != 6) return 2;
    const auto positions = take<float>(in, hdr[0] * 3);
    const auto vertex_data = take<sah_vertex_data>(in, hdr[0]);
    const auto indices = take<uint32_t>(in, hdr[1]);
    const auto primitives = take<sah_primitive>(in, hdr[2]);
    const auto materials = take<sah_material>(in, hdr[3]);
    using namespace sah;
    RenderBackend backend(0);
    RenderScene scene;
    scene.geometry.vertex_positions = upload(positions);
    scene.geometry.vertex_data = upload(vertex_data);
    scene.geometry.indices = upload(indices);
    scene.geometry.primitives = upload(primitives);
    scene.geometry.materials = upload(materials);
    scene.geometry.num_vertices = hdr[0];
    scene.geometry.num_indices = hdr[1];
    scene.geometry.num_primitives = hdr[2];
    scene.geometry.num_materials = hdr[3];
    SceneView view;  // start-up camera of the reference: scene_renderer.cpp:53-54,105-116
    view.rotate(0.f, 90.f * 3.14159265358979f / 180.f);
    view.set_position({-7.f, 1.f, 0.f});
    view.set_render_resolution(192, 108);
    view.set_perspective_projection(75.f, 192.f / 108.f, 0.05f);
    view.update_transforms();
    RenderGraph load{backend};
    const RenderScene::HostMesh host = {positions.data(), vertex_data.data(), hdr[0], indices.data(), hdr[1], primitives.data(), hdr[2],
                                        materials.data(), hdr[3], nullptr, false};
    scene.generate_emissive_point_clouds(load, host, hdr[4], hdr[5]);
    scene.generate_emissive_point_clouds(load, host, hdr[4], hdr[5]);  // nothing new: no second cloud per primitive
    load.finish();
    if (!load.get_errors().empty()) { fprintf(stderr, "pass failed: %s\n", load.get_errors()[0].c_str()); return 1; }
    LightPropagationVolume lpv(backend, 4, 1);
    lpv.update_cascade_transforms(view, scene.sun);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    const uint32_t clouds = (uint32_t)scene.emissive_clouds.size();
    fwrite(&clouds, 4, 1, out);
    fwrite(lpv.get_cascade_matrices(), sizeof(sah_lpv_cascade_matrices), 4, out);
    fwrite(lpv.get_cascade_bounds(), sizeof(sah_lpv_cascade_bounds), 4, out);
    std::vector<unsigned char> v((size_t)128 * 32 * 32 * 8);
    for (int frame = 0; frame < 3; frame++) {
        RenderGraph graph{backend};
        lpv.pre_render(graph, view, scene, nullptr);  // clears the volumes
        const uint32_t before = graph.get_num_passes();
        lpv.mesh_lights = frame == 1;
        if (frame < 2) lpv.inject_indirect_sun_light(graph, scene);
        else lpv.inject_emissive_point_clouds(graph, scene);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty()) return 1;
        const uint32_t passes = graph.get_num_passes() - before;
        fwrite(&passes, 4, 1, out);
        for (int c = 0; c < 3; c++) {
            backend.get_global_allocator().download(lpv.get_volume(c), v.data(), 128 * 8);
            fwrite(v.data(), 1, v.size(), out);
        }
    }
    fclose(out);
    return 0;
}
