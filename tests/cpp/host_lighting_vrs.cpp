// The VRSAA mode's two consumers through the C++ host façade (include/sah_host.hpp): LightingPhase::render with a shading-rate image, three
// times over one frame — as it is by default (the image ignored), after set_variable_rate_shading() (sah_lighting_vrs), and with the option
// set but no image passed — and VRSAA::resolve of the variable-rate frame.  The frame's planes (at twice the output resolution) and the
// shading-rate image come from a file written by tests/test_lighting_vrs_facade_gpu.py; the uniform blocks this program builds go back with
// the images, so that the test can make the direct calls on the very same blocks.
//
//   host_lighting_vrs <in.bin> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sah_host.hpp"

static std::vector<unsigned char> read_blob(FILE* f, size_t n) {
    std::vector<unsigned char> v(n);
    if (fread(v.data(), 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: host_lighting_vrs in.bin out.bin\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror("open input"); return 2; }
    uint32_t hdr[7];  // W, H of the frame (twice the output), sun mode, LPV steps, texel size x, y, depth tolerance (float bits)
    if (fread(hdr, 4, 7, in) != 7) return 2;
    const uint32_t W = hdr[0], H = hdr[1], sun_mode = hdr[2], lpv_steps = hdr[3];
    float tolerance;
    memcpy(&tolerance, &hdr[6], 4);
    if (W % 2 || H % 2) return 2;

    using namespace sah;
    RenderBackend backend(0);
    auto& alloc = backend.get_global_allocator();
    GBuffer gbuffer;
    gbuffer.color = alloc.create_texture("gbuffer_color", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
    gbuffer.normals = alloc.create_texture("gbuffer_normals", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    gbuffer.data = alloc.create_texture("gbuffer_data", SAH_FORMAT_R8G8B8A8_UNORM, W, H);
    gbuffer.emission = alloc.create_texture("gbuffer_emission", SAH_FORMAT_R8G8B8A8_SRGB, W, H);
    gbuffer.depth = alloc.create_texture("gbuffer_depth", SAH_FORMAT_D32_SFLOAT, W, H);
    TextureHandle ao = alloc.create_texture("ao", SAH_FORMAT_R32_SFLOAT, W, H);
    TextureHandle mask = alloc.create_texture("sun shadow mask", SAH_FORMAT_R32_SFLOAT, W, H);
    TextureHandle lit[3];
    for (int i = 0; i < 3; i++) lit[i] = alloc.create_texture("lit_scene", SAH_FORMAT_R16G16B16A16_SFLOAT, W, H);
    TextureHandle antialiased = alloc.create_texture("antialiased_scene", SAH_FORMAT_R16G16B16A16_SFLOAT, W / 2, H / 2);

    RenderScene scene;
    scene.sky.transmittance_lut = alloc.create_texture("Transmittance LUT", SAH_FORMAT_R16G16B16A16_SFLOAT, 256, 64);
    scene.sky.sky_view_lut = alloc.create_texture("Sky view LUT", SAH_FORMAT_R16G16B16A16_SFLOAT, 200, 200);
    scene.sun.set_shadow_mode((SunShadowMode)sun_mode);
    scene.sun.shadow_mask = mask;

    auto up = [&](TextureHandle t, uint32_t bpp) {
        auto blob = read_blob(in, (size_t)t->desc.width * t->desc.height * t->desc.depth * bpp);
        alloc.upload(t, blob.data(), t->desc.width * bpp);
    };
    up(gbuffer.color, 4); up(gbuffer.normals, 8); up(gbuffer.data, 4); up(gbuffer.emission, 4); up(gbuffer.depth, 4);
    up(ao, 4); up(mask, 4);
    up(scene.sky.transmittance_lut, 8); up(scene.sky.sky_view_lut, 8);

    SceneView view;  // start-up camera of the reference: scene_renderer.cpp:53-54,105-116
    view.rotate(0.f, 90.f * 3.14159265358979f / 180.f);
    view.set_position({-7.f, 1.f, 0.f});
    view.set_render_resolution(W, H);
    view.set_perspective_projection(75.f, (float)W / (float)H, 0.05f);
    view.update_transforms();

    LightPropagationVolume lpv(backend, 4, lpv_steps);
    lpv.update_cascade_transforms(view, scene.sun);
    for (int c = 0; c < 3; c++) up(lpv.get_volume(c), 8);  // stands in for RSM/VPL injection

    VRSAA vrsaa(alloc);
    vrsaa.set_max_shading_rate_texel_size(hdr[4], hdr[5]);
    vrsaa.set_shading_rates({{1, 1}, {1, 2}, {2, 1}, {2, 2}, {2, 4}, {4, 2}, {4, 4}});
    const uint32_t resolution[2] = {W, H};
    vrsaa.init(resolution);
    up(vrsaa.get_shading_rate_image(), 1);  // (stands in for generate_shading_rate_image over the last frame's contrast)
    fclose(in);

    RenderGraph graph{backend};
    NoiseTexture stbn_3d_unitvec, stbn_2d_scalar;
    IGlobalIlluminator* gi = &lpv;
    gi->post_render(graph, view, scene, gbuffer, stbn_3d_unitvec.get_layer(0));
    LightingPhase lighting;
    lighting.set_scene(scene);
    // 0: the default — the image is passed and ignored, the frame the façade has always written
    lighting.render(graph, view, gbuffer, lit[0], ao, gi, vrsaa.get_shading_rate_image(), stbn_3d_unitvec, stbn_2d_scalar.get_layer(0));
    // 1: the option set and the image passed: variable rate
    const auto texel = vrsaa.get_max_shading_rate_texel_size();
    lighting.set_variable_rate_shading(texel[0], texel[1], tolerance);
    lighting.render(graph, view, gbuffer, lit[1], ao, gi, vrsaa.get_shading_rate_image(), stbn_3d_unitvec, stbn_2d_scalar.get_layer(0));
    // 2: the option set, no image: full rate
    lighting.render(graph, view, gbuffer, lit[2], ao, gi, std::nullopt, stbn_3d_unitvec, stbn_2d_scalar.get_layer(0));
    vrsaa.resolve(graph, lit[1], antialiased);
    graph.finish();
    for (const auto& e : graph.get_errors()) fprintf(stderr, "pass failed: %s\n", e.c_str());
    if (!graph.get_errors().empty()) return 1;

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
    std::vector<unsigned char> buf((size_t)W * H * 8);
    for (int i = 0; i < 3; i++) {
        alloc.download(lit[i], buf.data(), W * 8);
        fwrite(buf.data(), 1, buf.size(), out);
    }
    alloc.download(antialiased, buf.data(), (W / 2) * 8);
    fwrite(buf.data(), 1, (size_t)(W / 2) * (H / 2) * 8, out);
    fclose(out);
    return 0;
}
