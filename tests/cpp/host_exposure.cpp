// Frames of auto-exposure through the C++ host façade (include/sah_host.hpp): AutoExposure::expose once per frame — the first frame, and
// the first of another extent, as "Auto-exposure: meter" then "Auto-exposure: apply", the others as the fused "Auto-exposure".  The
// frames' extents and scenes come from a file written by tests/test_exposure_gpu.py; each frame's state (16 bytes), histogram (256 words)
// and exposed plane go back.
//
//   host_exposure <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sah_host.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_exposure in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t frames;
    float adaptation;
    if (fread(&frames, 4, 1, in) != 1 || fread(&adaptation, 4, 1, in) != 1 || frames > 64) return 2;
    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    AutoExposure exposure(alloc);
    if (exposure.settings.key != 0.18f || exposure.settings.adaptation != 1.0f || exposure.get_exposed() || exposure.get_state()) return 1;  // the defaults; nothing made yet
    exposure.settings.adaptation = adaptation;
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    for (uint32_t frame = 0; frame < frames; frame++) {
        uint32_t extent[2];
        if (fread(extent, 4, 2, in) != 2 || !extent[0] || !extent[1] || extent[0] > 4096 || extent[1] > 4096) return 2;
        const uint32_t W = extent[0], H = extent[1];
        std::vector<unsigned char> px((size_t)W * H * 8);
        if (fread(px.data(), 1, px.size(), in) != px.size()) return 2;
        TextureHandle scene = alloc.create_texture("antialiased", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
        alloc.upload(scene, px.data(), W * 8);
        RenderGraph graph{backend};
        TextureHandle exposed = exposure.expose(graph, scene);
        graph.finish();
        for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
        if (!graph.get_errors().empty() || exposed != exposure.get_exposed()) return 1;
        sah_exposure_state state;
        uint32_t histogram[SAH_EXPOSURE_BINS];
        if (hipMemcpy(&state, exposure.get_state(), sizeof(state), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        if (hipMemcpy(histogram, exposure.get_histogram(), sizeof(histogram), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        alloc.download(exposed, px.data(), W * 8);
        fwrite(&state, sizeof(state), 1, out);
        fwrite(histogram, sizeof(histogram), 1, out);
        fwrite(px.data(), 1, px.size(), out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
