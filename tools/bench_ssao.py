"""Timings of sah_ssao (include/sah_ssao.h) on cuda:0 on the rasterised atrium at 1280 x 720, 2560 x 1440 and 3840 x 2160, without a blur
(the raw kernel alone) and with two blur passes (raw + blur kernel; "blur_added" is what the blur adds to a call, the difference of the two
medians, not a timing of k_ssao_blur: run the tool under a kernel trace for the kernels' own durations), with sah_rtao on the same
planes at the same resolutions in the same process: the alternative a caller has today for a real AO plane.  The acceleration structure
sah_rtao needs is built before the timing; its build time is reported separately.

    python tools/bench_ssao.py [--calls 30] [--rounds 7]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Prints one JSON line: milliseconds per call, GB/s over the algorithmic
bytes — 16 B/px without a blur (depth 4 + normals 8 read, AO 4 written; the taps' gathers hit the cache), + 8 B/px for the scratch plane's
round trip and + 4 B/px for the blur's depth with one — and that rate as a fraction of the 6.3 TB/s a copy kernel achieves on this device
(DESIGN.md §7)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ACHIEVABLE_BYTES_PER_S = 6.3e12
EXTENTS = {"720p": (1280, 720), "1440p": (2560, 1440), "4k": (3840, 2160)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    from androidrenderer_amd import _abi, frame, images, lib, mesh, scene

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = ctx.rt_build(geo)
    torch.cuda.synchronize()
    out["rt_build_ms_once"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["rt_triangles"] = stats[0]
    noise = torch.randint(0, 256, (128, 128, 4), dtype=torch.uint8, device="cuda")
    noise_p = images.plane(noise, _abi.FORMAT_R8G8B8A8_UNORM)
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    cases = {}
    for tag, (w, h) in EXTENTS.items():
        view = scene.SceneView.default(w, h)
        gb = {k: torch.zeros((h, w) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
        frame.rasterised_frame(ctx, geo, view.gpu_data, gb)
        torch.cuda.synchronize()
        ao, scratch = torch.zeros((h, w), dtype=torch.float32, device="cuda"), torch.zeros((h, w), dtype=torch.float32, device="cuda")
        d_, n_ = images.plane(gb["depth"], _abi.FORMAT_D32_SFLOAT), images.plane(gb["normals"], _abi.FORMAT_R16G16B16A16_SFLOAT)
        a_, s_ = images.plane(ao, _abi.FORMAT_R32_SFLOAT), images.plane(scratch, _abi.FORMAT_R32_SFLOAT)
        keep.append((view, gb, ao, scratch))
        out[f"{tag}_covered"] = round(float((gb["depth"] > 0).float().mean()), 3)
        p0, p2 = _abi.SsaoParams.default(blur_passes=0), _abi.SsaoParams.default()

        def raw(view=view, d_=d_, n_=n_, a_=a_, p0=p0):
            ctx.ssao(view.gpu_data, d_, n_, None, a_, p0)

        def blurred(view=view, d_=d_, n_=n_, s_=s_, a_=a_, p2=p2):
            ctx.ssao(view.gpu_data, d_, n_, s_, a_, p2)

        def rtao(view=view, d_=d_, n_=n_, a_=a_):
            ctx.rtao(view.gpu_data, d_, n_, noise_p, 1, 8.0, a_)
        cases[f"ssao_{tag}_blur0"] = (raw, 16 * w * h)
        cases[f"ssao_{tag}_blur2"] = (blurred, 28 * w * h)
        cases[f"rtao_{tag}"] = (rtao, None)
        blurred()
        torch.cuda.synchronize()
        out[f"{tag}_ao_mean"] = round(float(ao[gb["depth"] > 0].mean()), 4)
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
        if nbytes:
            out[f"{name}_gb_per_s"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
            out[f"{name}_of_achievable"] = round(nbytes / (ms * 1e-3) / ACHIEVABLE_BYTES_PER_S, 4)
    for tag, (w, h) in EXTENTS.items():
        out[f"blur_added_{tag}"] = round(out[f"ssao_{tag}_blur2"] - out[f"ssao_{tag}_blur0"], 5)
        out[f"rtao_over_ssao_blur2_{tag}"] = round(out[f"rtao_{tag}"] / out[f"ssao_{tag}_blur2"], 3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
