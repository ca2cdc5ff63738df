// Frames of camera motion blur through the C++ host façade (include/sah_host.hpp): MotionBlurPhase::render once per frame.  The frames'
// extents, jitters, settings and planes come from a file written by tests/test_motion_blur_facade_gpu.py; each frame's view block (as the
// façade's SceneView formed it: z_near and the two jitters are what the pass takes from it) and blurred plane go back.  A frame of other
// extents makes the phase re-create its textures.
//
//   host_motion_blur <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_motion_blur in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t frames;
    if (fread(&frames, 4, 1, in) != 1 || frames > 64) return 2;
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    MotionBlurPhase blur(alloc);
    const MotionBlurSettings d;
    if (d.shutter != 0.5f || d.max_blur_pixels != 32.0f || d.min_velocity_pixels != 0.5f || d.sample_count != 12 || d.depth_extent != 1.0f || d.dither ||
        blur.get_blurred())
        return 1;  // the header's defaults; nothing made yet
    SceneView view;
    view.set_position({-7.f, 1.f, 0.f});
    view.rotate(0.1f, 1.2f);
    {  // without planes the pass is recorded as a failure, not skipped
        RenderGraph graph{backend};
        if (blur.render(graph, view, nullptr, nullptr, nullptr) != nullptr) return 1;
        graph.finish();
        if (graph.get_errors().empty()) { fprintf(stderr, "a pass without planes did not fail\n"); return 1; }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    for (uint32_t frame = 0; frame < frames; frame++) {
        // output width, height, render width, height, dither, sample count; jitter x, y, shutter
        uint32_t head[6];
        float values[3];
        if (fread(head, 4, 6, in) != 6 || fread(values, 4, 3, in) != 3) return 2;
        for (int i = 0; i < 4; i++)
            if (!head[i] || head[i] > 4096) return 2;
        const uint32_t W = head[0], H = head[1], w = head[2], h = head[3];
        std::vector<unsigned char> scene((size_t)W * H * 8), depth((size_t)w * h * 4), vectors((size_t)w * h * 4);
        for (auto* v : {&scene, &depth, &vectors})
            if (fread(v->data(), 1, v->size(), in) != v->size()) return 2;
        TextureHandle scene_t = alloc.create_texture("scene", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        TextureHandle depth_t = alloc.create_texture("depth", SAH_FORMAT_D32_SFLOAT, w, h);
        TextureHandle vectors_t = alloc.create_texture("motion_vectors", SAH_FORMAT_R16G16_SFLOAT, w, h);
        alloc.upload(scene_t, scene.data(), W * 8);
        alloc.upload(depth_t, depth.data(), w * 4);
        alloc.upload(vectors_t, vectors.data(), w * 4);
        view.set_render_resolution(w, h);
        view.set_perspective_projection(75.f, (float)w / (float)h, 0.05f);
        view.set_jitter(values[0], values[1]);
        view.update_transforms();
        blur.settings.dither = head[4] != 0, blur.settings.sample_count = head[5], blur.settings.shutter = values[2];
        RenderGraph graph{backend};
        TextureHandle blurred = blur.render(graph, view, scene_t, depth_t, vectors_t);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty() || blurred != blur.get_blurred() || blurred->desc.width != W || blurred->desc.height != H) return 1;
        alloc.download(blurred, scene.data(), W * 8);
        fwrite(&view.get_gpu_data(), sizeof(sah_view_data), 1, out);
        fwrite(scene.data(), 1, scene.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
