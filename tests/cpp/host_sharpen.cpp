// Frames of contrast-adaptive sharpening through the C++ host façade (include/sah_host.hpp): Sharpener::sharpen once per frame, with a
// device exposure state of the test's making on the frames that ask for one.  The frames' extents, settings and scenes come from a file
// written by tests/test_sharpen_gpu.py; each frame's sharpened plane goes back.
//
//   host_sharpen <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_sharpen in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t frames;
    if (fread(&frames, 4, 1, in) != 1 || frames > 64) return 2;
    using namespace sah;
    if (SharpenSettings::from_stops(0.0f) != 1.0f || SharpenSettings::from_stops(1.0f) != 0.5f || SharpenSettings::from_stops(2.0f) != 0.25f ||
        SharpenSettings::from_stops(-3.0f) != 1.0f || SharpenSettings::from_stops(1.0e9f) != 0.0f)
        return 1;  // the stops convention: full at 0, halved per stop, clamped into [0, 1]
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    Sharpener sharpener(alloc);
    if (sharpener.settings.sharpness != 1.0f || sharpener.settings.pre_scale != 1.0f || sharpener.settings.denoise || sharpener.get_sharpened()) return 1;  // the defaults; nothing made yet
    TextureHandle state = alloc.create_texture("exposure state", SAH_FORMAT_R32_SFLOAT, 4, 1);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    for (uint32_t frame = 0; frame < frames; frame++) {
        // width, height, denoise, with_exposure; stops, pre_scale, exposure
        uint32_t head[4];
        float values[3];
        if (fread(head, 4, 4, in) != 4 || fread(values, 4, 3, in) != 3 || !head[0] || !head[1] || head[0] > 4096 || head[1] > 4096) return 2;
        const uint32_t W = head[0], H = head[1];
        std::vector<unsigned char> px((size_t)W * H * 8);
        if (fread(px.data(), 1, px.size(), in) != px.size()) return 2;
        TextureHandle scene = alloc.create_texture("upscaled", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        alloc.upload(scene, px.data(), W * 8);
        const float state_words[4] = {values[2], 0.0f, 0.0f, 0.0f};
        alloc.upload(state, state_words, 16);
        sharpener.settings.sharpness = SharpenSettings::from_stops(values[0]);
        sharpener.settings.pre_scale = values[1];
        sharpener.settings.denoise = head[2] != 0;
        RenderGraph graph{backend};
        TextureHandle sharpened = sharpener.sharpen(graph, scene, head[3] ? static_cast<const sah_exposure_state*>(state->desc.ptr) : nullptr);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty() || sharpened != sharpener.get_sharpened() || sharpened->desc.width != W || sharpened->desc.height != H) return 1;
        alloc.download(sharpened, px.data(), W * 8);
        fwrite(px.data(), 1, px.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
