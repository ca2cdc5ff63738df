"""Timings of sah_rt_denoise (include/sah_rt_denoise.h) on cuda:0 on the rasterised atrium at 1280 x 720, 2560 x 1440 and 3840 x 2160 with a
history (a static camera: one history tap per pixel), with passes = 0 (the temporal kernel alone, which then writes `denoised` too) and
passes = 3 (temporal + filter kernel; "filter_added" is the difference of the two medians, not a timing of k_rd_filter: run the tool
under a kernel trace for the kernels' own durations), alternating in the same process with sah_copy_scene at the same extent — the
achievable-rate yardstick: 8 B read and 8 B written per pixel by a kernel that does nothing else.

    python tools/bench_rt_denoise.py [--calls 30] [--rounds 7] [--sizes 720p,1440p,4k]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Prints one JSON line: milliseconds per call, GB/s over the pass's own
bytes — the temporal kernel reads 30 B/px (sample 4, depth 4, normals 8, motion vector 4, previous depth 4, history 4, length 2) and writes
6 (10 with passes = 0), the filter reads 16 (depth 4, normals 8, accum 4; the halo's second reads hit the cache) and writes 4 — and that
rate as a fraction of the rate sah_copy_scene reached at the same extent in the same run.  The noisy plane is sah_rtao's."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXTENTS = {"720p": (1280, 720), "1440p": (2560, 1440), "4k": (3840, 2160)}
BYTES = {0: 30 + 10, 3: 30 + 6 + 16 + 4}  # per pixel, by passes
COPY_BYTES = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="720p,1440p,4k")
    args = ap.parse_args()
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
    R32F, D32, R16F = _abi.FORMAT_R32_SFLOAT, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16_SFLOAT
    cases = {}
    sizes = [s for s in args.sizes.split(",") if s]
    for tag in sizes:
        w, h = EXTENTS[tag]
        view = scene.SceneView.default(w, h)
        view.update_transforms()
        gb = {k: torch.zeros((h, w) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
        mv = torch.zeros((h, w, 2), dtype=torch.int16, device="cuda")
        frame.rasterised_frame(ctx, geo, view.gpu_data, gb, motion_vectors=mv)
        f32 = lambda: torch.zeros((h, w), dtype=torch.float32, device="cuda")  # noqa: E731
        f16 = lambda: torch.zeros((h, w), dtype=torch.float16, device="cuda")  # noqa: E731
        noisy, previous_depth, accum, denoised, lengths = f32(), gb["depth"].clone(), [f32(), f32()], f32(), [f16(), f16()]
        d_, n_ = images.plane(gb["depth"], D32), images.plane(gb["normals"], _abi.FORMAT_R16G16B16A16_SFLOAT)
        ctx.rtao(view.gpu_data, d_, n_, images.plane(noise, _abi.FORMAT_R8G8B8A8_UNORM), 1, 8.0, images.plane(noisy, R32F))
        common = dict(noisy=images.plane(noisy, R32F), depth=d_, normals=n_, motion_vectors=images.plane(mv, _abi.FORMAT_R16G16_SFLOAT),
                      accum_out=images.plane(accum[1], R32F), length_out=images.plane(lengths[1], R16F), denoised=images.plane(denoised, R32F))
        first = _abi.RtDenoiseDesc.of(**dict(common, accum_out=images.plane(accum[0], R32F), length_out=images.plane(lengths[0], R16F)))
        ctx.rt_denoise(view.gpu_data, first, _abi.RtDenoiseParams.default(flags=_abi.RT_DENOISE_HISTORY_INVALID))  # the history of the timed calls
        desc = _abi.RtDenoiseDesc.of(previous_depth=images.plane(previous_depth, D32), history=images.plane(accum[0], R32F),
                                     history_length=images.plane(lengths[0], R16F), **common)
        lit, aa = (torch.zeros((h, w, 4), dtype=torch.int16, device="cuda") for _ in range(2))
        l_, a_ = images.plane(lit, _abi.FORMAT_R16G16B16A16_SFLOAT), images.plane(aa, _abi.FORMAT_R16G16B16A16_SFLOAT)
        keep.append((view, gb, mv, noisy, previous_depth, accum, denoised, lengths, lit, aa, first, desc))
        torch.cuda.synchronize()
        out[f"{tag}_covered"] = round(float((gb["depth"] > 0).float().mean()), 3)
        for passes in (0, 3):
            p = _abi.RtDenoiseParams.default(passes=passes)

            def denoise(view=view, desc=desc, p=p):
                ctx.rt_denoise(view.gpu_data, desc, p)
            cases[f"rt_denoise_{tag}_passes{passes}"] = (denoise, BYTES[passes] * w * h)

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
            out[f"rt_denoise_{tag}_passes{passes}_of_copy_rate"] = round(out[f"rt_denoise_{tag}_passes{passes}_gb_per_s"] / out[f"copy_scene_{tag}_gb_per_s"], 4)
        out[f"filter_added_{tag}"] = round(out[f"rt_denoise_{tag}_passes3"] - out[f"rt_denoise_{tag}_passes0"], 5)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
