"""Timings of sah_rtgi_denoise (include/sah_rtgi_denoise.h) on cuda:0 on the rasterised atrium at 1280 x 720, 2560 x 1440 and 3840 x 2160
with a history (a static camera: one history tap per pixel), with passes = 0 (the temporal kernel alone, which then writes the two
denoised planes too) and passes = 3 (temporal + filter kernel; "filter_added" is the difference of the two medians, not a timing of
k_gd_filter: run the tool under a kernel trace for the kernels' own durations), alternating in the same process with sah_rt_denoise on
the same G-buffer — the yardstick: the one-channel sibling at the same extents in the same run — and with sah_copy_scene, the
achievable-rate yardstick: 8 B read and 8 B written per pixel by a kernel that does nothing else.

    python tools/bench_rtgi_denoise.py [--calls 30] [--rounds 7] [--sizes 720p,1440p,4k]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Prints one JSON line: milliseconds per call, GB/s over the pass's own
bytes — the temporal kernel reads 60 B/px (ray 8, irradiance 8, depth 4, normals 8, motion vector 4, previous depth 4, history 16, moments
8) and writes 24 (40 with passes = 0), the filter reads 40 (depth 4, normals 8, accum 16, moments 8, the dword of the ray that holds its
distance 4; the halo's second reads hit the cache) and writes 16 — that rate as a fraction of the rate sah_copy_scene reached at the same
extent in the same run, and the temporal kernel's as a fraction of the 8 TB/s HBM peak.  The ray planes are synthetic (a direction in the
hemisphere, an irradiance that is 0 for 70 % of the pixels): no branch of the pass depends on their values."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXTENTS = {"720p": (1280, 720), "1440p": (2560, 1440), "4k": (3840, 2160)}
TEMPORAL_READ, TEMPORAL_WRITE, FILTER_READ, FILTER_WRITE = 60, 24, 40, 16  # bytes per pixel
BYTES = {0: TEMPORAL_READ + TEMPORAL_WRITE + 16, 3: TEMPORAL_READ + TEMPORAL_WRITE + FILTER_READ + FILTER_WRITE}
MASK_BYTES = {0: 30 + 10, 3: 30 + 6 + 16 + 4}  # sah_rt_denoise's (tools/bench_rt_denoise.py)
COPY_BYTES = 16
HBM_PEAK_GB_PER_S = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="720p,1440p,4k")
    args = ap.parse_args()
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, frame, images, lib, mesh, scene

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(lib.LIB_PATH)}
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    ctx.rt_build(geo)
    noise = torch.randint(0, 256, (128, 128, 4), dtype=torch.uint8, device="cuda")
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    R32F, D32, R16F, RGBA16F = _abi.FORMAT_R32_SFLOAT, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16_SFLOAT, _abi.FORMAT_R16G16B16A16_SFLOAT
    RGBA32F, RG32F = _abi.FORMAT_R32G32B32A32_SFLOAT, _abi.FORMAT_R32G32_SFLOAT
    cases = {}
    sizes = [s for s in args.sizes.split(",") if s]
    g = np.random.default_rng(1)
    for tag in sizes:
        w, h = EXTENTS[tag]
        view = scene.SceneView.default(w, h)
        view.update_transforms()
        gb = {k: torch.zeros((h, w) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
        mv = torch.zeros((h, w, 2), dtype=torch.int16, device="cuda")
        frame.rasterised_frame(ctx, geo, view.gpu_data, gb, motion_vectors=mv)
        d_, n_, m_ = images.plane(gb["depth"], D32), images.plane(gb["normals"], RGBA16F), images.plane(mv, _abi.FORMAT_R16G16_SFLOAT)
        previous_depth = gb["depth"].clone()
        # one ray a pixel: a direction in the hemisphere of +z and +x, an irradiance that is 0 for 70 % of the pixels
        d = g.normal(0, 1, (h, w, 3)).astype(np.float32)
        d[..., 2], d[..., 0] = np.abs(d[..., 2]) + 0.2, np.abs(d[..., 0])
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        rays = torch.from_numpy(np.concatenate([d, g.uniform(0.1, 30, (h, w, 1))], -1).astype(np.float16).view(np.int16)).cuda()
        e = (g.random((h, w, 1)) < 0.3) * g.uniform(0.01, 0.1, (h, w, 1)) * np.array([1.0, 0.8, 0.6, 0.0])
        irr = torch.from_numpy(e.astype(np.float16).view(np.int16)).cuda()
        z4 = lambda c, t=torch.float32: torch.zeros((h, w, c), dtype=t, device="cuda")  # noqa: E731
        accum, moments, orb, oir = [z4(4), z4(4)], [z4(2), z4(2)], z4(4, torch.int16), z4(4, torch.int16)
        common = dict(ray_buffer=images.plane(rays, RGBA16F), ray_irradiance=images.plane(irr, RGBA16F), depth=d_, normals=n_, motion_vectors=m_,
                      accum_out=images.plane(accum[1], RGBA32F), moments_out=images.plane(moments[1], RG32F),
                      denoised_ray_buffer=images.plane(orb, RGBA16F), denoised_irradiance=images.plane(oir, RGBA16F))
        first = _abi.RtgiDenoiseDesc.of(**dict(common, accum_out=images.plane(accum[0], RGBA32F), moments_out=images.plane(moments[0], RG32F)))
        ctx.rtgi_denoise(view.gpu_data, first, _abi.RtgiDenoiseParams.default(flags=_abi.RTGI_DENOISE_HISTORY_INVALID))  # the history of the timed calls
        desc = _abi.RtgiDenoiseDesc.of(previous_depth=images.plane(previous_depth, D32), history=images.plane(accum[0], RGBA32F),
                                       history_moments=images.plane(moments[0], RG32F), **common)
        # the one-channel sibling on the same G-buffer
        f32 = lambda: torch.zeros((h, w), dtype=torch.float32, device="cuda")  # noqa: E731
        f16 = lambda: torch.zeros((h, w), dtype=torch.float16, device="cuda")  # noqa: E731
        noisy, maccum, mdenoised, mlengths = f32(), [f32(), f32()], f32(), [f16(), f16()]
        ctx.rtao(view.gpu_data, d_, n_, images.plane(noise, _abi.FORMAT_R8G8B8A8_UNORM), 1, 8.0, images.plane(noisy, R32F))
        mcommon = dict(noisy=images.plane(noisy, R32F), depth=d_, normals=n_, motion_vectors=m_, accum_out=images.plane(maccum[1], R32F),
                       length_out=images.plane(mlengths[1], R16F), denoised=images.plane(mdenoised, R32F))
        mfirst = _abi.RtDenoiseDesc.of(**dict(mcommon, accum_out=images.plane(maccum[0], R32F), length_out=images.plane(mlengths[0], R16F)))
        ctx.rt_denoise(view.gpu_data, mfirst, _abi.RtDenoiseParams.default(flags=_abi.RT_DENOISE_HISTORY_INVALID))
        mdesc = _abi.RtDenoiseDesc.of(previous_depth=images.plane(previous_depth, D32), history=images.plane(maccum[0], R32F),
                                      history_length=images.plane(mlengths[0], R16F), **mcommon)
        lit, aa = z4(4, torch.int16), z4(4, torch.int16)
        l_, a_ = images.plane(lit, RGBA16F), images.plane(aa, RGBA16F)
        keep.append((view, gb, mv, previous_depth, rays, irr, accum, moments, orb, oir, first, desc, noisy, maccum, mdenoised, mlengths, mfirst, mdesc, lit, aa))
        torch.cuda.synchronize()
        out[f"{tag}_covered"] = round(float((gb["depth"] > 0).float().mean()), 3)
        for passes in (0, 3):
            p, mp = _abi.RtgiDenoiseParams.default(passes=passes), _abi.RtDenoiseParams.default(passes=passes)

            def denoise(view=view, desc=desc, p=p):
                ctx.rtgi_denoise(view.gpu_data, desc, p)

            def mask(view=view, mdesc=mdesc, mp=mp):
                ctx.rt_denoise(view.gpu_data, mdesc, mp)
            cases[f"rtgi_denoise_{tag}_passes{passes}"] = (denoise, BYTES[passes] * w * h)
            cases[f"rt_denoise_{tag}_passes{passes}"] = (mask, MASK_BYTES[passes] * w * h)

        def copy(l_=l_, a_=a_):
            ctx.copy_scene(l_, a_)
        cases[f"copy_scene_{tag}"] = (copy, COPY_BYTES * w * h)
    times = {k: [] for k in cases}
    for fn, _ in cases.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, (fn, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.calls)
    for name, (_, nbytes) in cases.items():
        ms = statistics.median(times[name])
        out[name] = round(ms, 5)
        out[f"{name}_range"] = round(max(times[name]) - min(times[name]), 5)
        out[f"{name}_gb_per_s"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
    for tag in sizes:
        for passes in (0, 3):
            k = f"rtgi_denoise_{tag}_passes{passes}"
            out[f"{k}_of_copy_rate"] = round(out[f"{k}_gb_per_s"] / out[f"copy_scene_{tag}_gb_per_s"], 4)
            out[f"{k}_times_rt_denoise"] = round(out[k] / out[f"rt_denoise_{tag}_passes{passes}"], 3)
        out[f"temporal_{tag}_of_hbm_peak"] = round(out[f"rtgi_denoise_{tag}_passes0_gb_per_s"] / HBM_PEAK_GB_PER_S, 4)
        out[f"filter_added_{tag}"] = round(out[f"rtgi_denoise_{tag}_passes3"] - out[f"rtgi_denoise_{tag}_passes0"], 5)
    out["bytes_per_pixel"] = {"temporal_read": TEMPORAL_READ, "temporal_write": TEMPORAL_WRITE, "temporal_write_passes0": TEMPORAL_WRITE + 16,
                              "filter_read": FILTER_READ, "filter_write": FILTER_WRITE}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
