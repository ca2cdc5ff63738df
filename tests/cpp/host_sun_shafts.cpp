// Frames of volumetric sun light through the C++ host façade (include/sah_host.hpp): SunShafts::render once per frame.  The frames' extents,
// settings, planes and shadow maps come from a file written by tests/test_sun_shafts_facade_gpu.py; each frame's view block and sun
// constants (as the façade's SceneView and DirectionalLight formed them), the step transmittance the façade made of the extinction, and the
// output and march planes go back.  A frame of another extent or downscale makes the object re-create its textures.
//
//   host_sun_shafts <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_sun_shafts in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t frames;
    if (fread(&frames, 4, 1, in) != 1 || frames > 64) return 2;
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    SunShafts shafts(alloc);
    const SunShaftsSettings d;
    if (d.step_length != 0.5f || d.num_steps != 32 || d.anisotropy != 0.6f || d.depth_bias != 0.0005f || d.depth_sharpness != 50.0f || d.downscale != 1 || d.dither ||
        d.albedo[1] != 0.00031415927f || d.ambient[2] != 0.0f || shafts.get_output() || shafts.get_march())
        return 1;  // the header's defaults; nothing made yet
    SceneView view;
    view.set_position({-7.f, 1.f, 0.f});
    view.rotate(0.f, 1.5707964f);
    DirectionalLight sun;
    sun.set_shadow_mode(SunShadowMode::CascadedShadowMaps);
    {  // without planes the pass is recorded as a failure, not skipped
        RenderGraph graph{backend};
        if (shafts.render(graph, view, sun, nullptr, nullptr) != nullptr) return 1;
        graph.finish();
        if (graph.get_errors().empty()) { fprintf(stderr, "a pass without planes did not fail\n"); return 1; }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    for (uint32_t frame = 0; frame < frames; frame++) {
        // width, height, downscale, dither, steps, map resolution, map layers (0: no map), map is D32; extinction, step length, ambient
        uint32_t head[8];
        float values[3];
        if (fread(head, 4, 8, in) != 8 || fread(values, 4, 3, in) != 3) return 2;
        const uint32_t w = head[0], h = head[1], res = head[5], layers = head[6];
        if (!w || w > 4096 || !h || h > 4096 || res > 4096 || layers > 4) return 2;
        const uint32_t map_bpp = head[7] ? 4 : 2;
        std::vector<unsigned char> depth((size_t)w * h * 4), lit((size_t)w * h * 8), map((size_t)res * res * layers * map_bpp);
        for (auto* v : {&depth, &lit, &map})
            if (!v->empty() && fread(v->data(), 1, v->size(), in) != v->size()) return 2;
        TextureHandle depth_t = alloc.create_texture("depth", SAH_FORMAT_D32_SFLOAT, w, h);
        TextureHandle lit_t = alloc.create_texture("lit", SAH_FORMAT_R16G16B16A16_SFLOAT, w, h);
        alloc.upload(depth_t, depth.data(), w * 4);
        alloc.upload(lit_t, lit.data(), w * 8);
        sun.shadowmap_handle = nullptr;
        if (layers) {
            sun.shadowmap_handle = alloc.create_texture("shadowmap", head[7] ? SAH_FORMAT_D32_SFLOAT : SAH_FORMAT_D16_UNORM, res, res, layers);
            alloc.upload(sun.shadowmap_handle, map.data(), res * map_bpp);
        }
        view.set_render_resolution(w, h);
        view.set_perspective_projection(75.f, (float)w / (float)h, 0.05f);
        view.rotate(0.f, 0.1f);
        view.update_transforms();
        sun.update_shadow_cascades(view, 4, 32.f, 0.95f, res ? res : 64);
        shafts.settings.downscale = head[2], shafts.settings.dither = head[3] != 0, shafts.settings.num_steps = head[4];
        shafts.settings.extinction = values[0], shafts.settings.step_length = values[1];
        for (int i = 0; i < 3; i++) shafts.settings.ambient[i] = values[2];
        RenderGraph graph{backend};
        TextureHandle result = shafts.render(graph, view, sun, depth_t, lit_t);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty() || result != shafts.get_output() || result->desc.width != w || result->desc.height != h) return 1;
        TextureHandle march = shafts.get_march();
        const uint32_t mw = (w + head[2] - 1) / head[2], mh = (h + head[2] - 1) / head[2];
        if (!march || march->desc.width != mw || march->desc.height != mh) return 1;
        std::vector<unsigned char> march_bytes((size_t)mw * mh * 8);
        alloc.download(result, lit.data(), w * 8);
        alloc.download(march, march_bytes.data(), mw * 8);
        const float tau = shafts.settings.step_transmittance();
        fwrite(&view.get_gpu_data(), sizeof(sah_view_data), 1, out);
        fwrite(&sun.get_constants(), sizeof(sah_sun_light_constants), 1, out);
        fwrite(&tau, 4, 1, out);
        fwrite(lit.data(), 1, lit.size(), out);
        fwrite(march_bytes.data(), 1, march_bytes.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
