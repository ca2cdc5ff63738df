"""Timings of sah_sharpen (include/sah_sharpen.h) on cuda:0 at 1280 x 720, 2560 x 1440 and 3840 x 2160 on the blocky image of
tests/sharpen_ref.py (every pixel eligible, the lobe at work almost everywhere): plain, with SAH_SHARPEN_DENOISE, and with a device exposure
state; in the same process at the same extents sah_exposure_apply, which moves the same bytes in and out with no neighbourhood, and
sah_taa_resolve, which has the same tile shape and more work; and the pipeline the pass exists for — sah_taa_upscale from 2560 x 1440 to
3840 x 2160 followed by sah_sharpen at 3840 x 2160 — against sah_taa_resolve at 3840 x 2160 alone.

    python tools/bench_sharpen.py [--calls 30] [--rounds 7]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Prints one JSON line: milliseconds per call, GB/s over the algorithmic
bytes — 8 B/px read and 8 B/px written — and that rate as a fraction of the 6.3 TB/s a copy kernel achieves on this device."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ACHIEVABLE_BYTES_PER_S = 6.3e12
EXTENTS = {"720p": (1280, 720), "1440p": (2560, 1440), "4k": (3840, 2160)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, images, lib
    from tests import sharpen_ref as ref

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT
    keep, cases, planes = [], {}, {}
    for tag, (w, h) in EXTENTS.items():
        scene = torch.from_numpy(ref.blocky_inputs(w, h, 5).view(np.int16)).cuda()
        sharpened = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
        state = torch.zeros(4, dtype=torch.float32, device="cuda")
        state[0] = 0.5
        depth = torch.rand((h, w), dtype=torch.float32, device="cuda")
        mv = torch.zeros((h, w, 2), dtype=torch.float16, device="cuda")
        history = scene.clone()
        keep.append((scene, sharpened, state, depth, mv, history))
        scene_p, out_p, st = images.plane(scene, RGBA16F), images.plane(sharpened, RGBA16F), state.data_ptr()
        depth_p, mv_p, hist_p = images.plane(depth, _abi.FORMAT_D32_SFLOAT), images.plane(mv, _abi.FORMAT_R16G16_SFLOAT), images.plane(history, RGBA16F)
        planes[tag] = (scene_p, depth_p, mv_p, hist_p, out_p)
        plain, denoise = _abi.SharpenParams.default(), _abi.SharpenParams.default(flags=_abi.SHARPEN_DENOISE)
        taa = _abi.TaaParams()
        taa.blend, taa.flags = 0.1, _abi.TAA_HDR_WEIGHTS
        cases[f"sharpen_{tag}"] = (lambda scene_p=scene_p, out_p=out_p, plain=plain: ctx.sharpen(scene_p, None, out_p, plain), 16 * w * h)
        cases[f"sharpen_denoise_{tag}"] = (lambda scene_p=scene_p, out_p=out_p, denoise=denoise: ctx.sharpen(scene_p, None, out_p, denoise), 16 * w * h)
        cases[f"sharpen_exposure_{tag}"] = (lambda scene_p=scene_p, out_p=out_p, st=st, plain=plain: ctx.sharpen(scene_p, st, out_p, plain), 16 * w * h)
        cases[f"exposure_apply_{tag}"] = (lambda scene_p=scene_p, out_p=out_p, st=st: ctx.exposure_apply(scene_p, st, out_p), 16 * w * h)
        cases[f"taa_resolve_{tag}"] = (lambda scene_p=scene_p, depth_p=depth_p, mv_p=mv_p, hist_p=hist_p, out_p=out_p, taa=taa:
                                       ctx.taa_resolve(scene_p, depth_p, mv_p, hist_p, out_p, taa), None)
        ctx.sharpen(scene_p, None, out_p, plain)
        torch.cuda.synchronize()
        out[f"{tag}_pixels_changed"] = round(float((sharpened[..., :3] != scene[..., :3]).any(-1).float().mean()), 4)
    # the pipeline: 1440p -> 4K upscale, then sharpen at 4K (the upscale's output is the sharpening's input)
    lit_p, depth_p, mv_p = planes["1440p"][:3]
    hist4k_p = planes["4k"][3]
    upscaled, final = (torch.zeros((2160, 3840, 4), dtype=torch.int16, device="cuda") for _ in range(2))
    keep.append((upscaled, final))
    up_p, final_p = images.plane(upscaled, RGBA16F), images.plane(final, RGBA16F)
    up = _abi.TaaUpscaleParams()
    up.blend, up.min_confidence, up.flags = 0.1, 0.05, _abi.TAA_HDR_WEIGHTS
    up.jitter[:] = [0.25, -0.125]
    up.previous_jitter[:] = [-0.25, 0.375]
    plain = _abi.SharpenParams.default()

    def upscale():
        ctx.taa_upscale(lit_p, depth_p, mv_p, hist4k_p, up_p, up)

    def upscale_and_sharpen():
        ctx.taa_upscale(lit_p, depth_p, mv_p, hist4k_p, up_p, up)
        ctx.sharpen(up_p, None, final_p, plain)
    cases["upscale_1440p_to_4k"] = (upscale, None)
    cases["upscale_1440p_to_4k_and_sharpen"] = (upscale_and_sharpen, None)
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
            out[f"{name}_floor_ms"] = round(nbytes / ACHIEVABLE_BYTES_PER_S * 1e3, 5)
            out[f"{name}_gb_per_s"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
            out[f"{name}_of_achievable"] = round(nbytes / (ms * 1e-3) / ACHIEVABLE_BYTES_PER_S, 4)
    for tag in EXTENTS:
        out[f"sharpen_over_exposure_apply_{tag}"] = round(out[f"sharpen_{tag}"] / out[f"exposure_apply_{tag}"], 3)
        out[f"sharpen_over_taa_resolve_{tag}"] = round(out[f"sharpen_{tag}"] / out[f"taa_resolve_{tag}"], 3)
        out[f"denoise_over_plain_{tag}"] = round(out[f"sharpen_denoise_{tag}"] / out[f"sharpen_{tag}"], 3)
    out["upscale_and_sharpen_over_taa_resolve_4k"] = round(out["upscale_1440p_to_4k_and_sharpen"] / out["taa_resolve_4k"], 3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
