// Frames of screen-space reflections through the C++ host façade (include/sah_host.hpp): ScreenSpaceReflections::render once per frame,
// taking its reflections from the lit scene itself or, on the frames that ask for it, from a copy of the frame before's output.  The
// frames' extents, jitters, settings and planes come from a file written by tests/test_ssr_facade_gpu.py; each frame's view block (as the
// façade's SceneView formed it) and reflected plane go back.  A frame of another extent makes the phase re-create its textures.
//
//   host_ssr <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_ssr in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t frames;
    if (fread(&frames, 4, 1, in) != 1 || frames > 64) return 2;
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    ScreenSpaceReflections ssr(alloc);
    const SsrSettings d;
    if (d.max_distance != 50.0f || d.thickness != 0.5f || d.stride_pixels != 4.0f || d.max_steps != 64 || d.refine_steps != 4 || d.max_roughness != 0.6f ||
        d.edge_fade != 0.1f || d.intensity != 1.0f || d.jitter || d.reflection_only || ssr.get_reflected())
        return 1;  // the header's defaults; nothing made yet
    SceneView view;
    view.set_position({-7.f, 1.f, 0.f});
    view.rotate(0.1f, 1.2f);
    {  // without a lit scene the pass is recorded as a failure, not skipped
        RenderGraph graph{backend};
        if (ssr.render(graph, view, GBuffer{}, nullptr) != nullptr) return 1;
        graph.finish();
        if (graph.get_errors().empty()) { fprintf(stderr, "a pass without planes did not fail\n"); return 1; }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    TextureHandle previous = nullptr;
    for (uint32_t frame = 0; frame < frames; frame++) {
        // width, height, from the previous output, jitter flag, reflection only; jitter x, y, stride, thickness
        uint32_t head[5];
        float values[4];
        if (fread(head, 4, 5, in) != 5 || fread(values, 4, 4, in) != 4 || !head[0] || !head[1] || head[0] > 4096 || head[1] > 4096) return 2;
        const uint32_t W = head[0], H = head[1];
        const size_t n = (size_t)W * H;
        std::vector<unsigned char> color(n * 4), normals(n * 8), data(n * 4), depth(n * 4), lit(n * 8);
        for (auto* v : {&color, &normals, &data, &depth, &lit})
            if (fread(v->data(), 1, v->size(), in) != v->size()) return 2;
        GBuffer gbuffer;
        gbuffer.color = alloc.create_texture("gbuffer_color", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
        gbuffer.normals = alloc.create_texture("gbuffer_normals", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        gbuffer.data = alloc.create_texture("gbuffer_data", SAH_FORMAT_R8G8B8A8_UNORM, W, H);
        gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
        TextureHandle lit_scene = alloc.create_texture("lit_scene", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        alloc.upload(gbuffer.color, color.data(), W * 4);
        alloc.upload(gbuffer.normals, normals.data(), W * 8);
        alloc.upload(gbuffer.data, data.data(), W * 4);
        alloc.upload(gbuffer.depth, depth.data(), W * 4);
        alloc.upload(lit_scene, lit.data(), W * 8);
        if (head[2] && (!previous || previous->desc.width != W || previous->desc.height != H)) return 2;
        view.set_render_resolution(W, H);
        view.set_perspective_projection(75.f, (float)W / (float)H, 0.05f);
        view.set_jitter(values[0], values[1]);
        view.update_transforms();
        ssr.settings.jitter = head[3] != 0, ssr.settings.reflection_only = head[4] != 0;
        ssr.settings.stride_pixels = values[2], ssr.settings.thickness = values[3];
        RenderGraph graph{backend};
        TextureHandle reflected = ssr.render(graph, view, gbuffer, lit_scene, head[2] ? previous : nullptr);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty() || reflected != ssr.get_reflected() || reflected->desc.width != W || reflected->desc.height != H) return 1;
        alloc.download(reflected, lit.data(), W * 8);
        fwrite(&view.get_gpu_data(), sizeof(sah_view_data), 1, out);
        fwrite(lit.data(), 1, lit.size(), out);
        previous = alloc.create_texture("previous output", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);  // a copy: the phase writes its own texture next frame
        alloc.upload(previous, lit.data(), W * 8);
    }
    fclose(in);
    fclose(out);
    return 0;
}
