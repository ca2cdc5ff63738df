"""Timings of the two VRSAA passes (include/sah_vrsaa.h) on cuda:0 at 7680 x 4320 and 3840 x 2160, the shading-rate image with a 16 x 16
and an 8 x 8 texel size, with sah_copy_scene at the same extent in the same process as the yardstick (16 B/px; DESIGN.md §5 gives it 67 %
of HBM).

    python tools/bench_vrsaa.py [--calls 50] [--rounds 7]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Prints one JSON line: milliseconds per call and the HBM fraction by
algorithmic bytes over 8 TB/s — 12 B/px for the contrast pass (4 colour + 4 depth read, 4 written), 4 B per contrast texel + 1 B per
output texel for the shading-rate image, 16 B/px for the copy."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
RATES = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (4, 2), (4, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    from androidrenderer_amd import _abi, images, lib, scene

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    for (W, H, tag) in ((7680, 4320, "8k"), (3840, 2160, "4k")):
        g = torch.Generator(device="cuda").manual_seed(1)
        color = torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device="cuda", generator=g)
        depth = torch.rand((H, W), dtype=torch.float32, device="cuda", generator=g)
        contrast = torch.zeros((H, W, 2), dtype=torch.int16, device="cuda")
        lit = torch.randint(0, 0x3c00, (H, W, 4), dtype=torch.int16, device="cuda", generator=g)
        aa = torch.zeros_like(lit)
        C_, D_, O_ = images.plane(color, _abi.FORMAT_R8G8B8A8_SRGB), images.plane(depth, _abi.FORMAT_D32_SFLOAT), images.plane(contrast, _abi.FORMAT_R16G16_SFLOAT)
        L_, A_ = images.plane(lit, _abi.FORMAT_R16G16B16A16_SFLOAT), images.plane(aa, _abi.FORMAT_R16G16B16A16_SFLOAT)
        cases = {"contrast": (lambda: ctx.vrsaa_measure_aliasing(C_, D_, O_), 12 * W * H), "copy_scene": (lambda: ctx.copy_scene(L_, A_), 16 * W * H)}
        keep = []
        for texel in (16, 8):
            sw, sh = scene.shading_rate_image_extent((W, H), (texel, texel))
            sri = torch.zeros((sh, sw), dtype=torch.uint8, device="cuda")
            S_, P_ = images.plane(sri, _abi.FORMAT_R8_UINT), scene.shading_rate_params((W, H), (sw, sh), RATES)
            keep.append((sri, S_, P_))
            cases[f"shading_rate_{texel}"] = ((lambda S=S_, P=P_: ctx.vrsaa_shading_rate_image(O_, S, P)), 4 * W * H + sw * sh)
        times = {k: [] for k in cases}
        for fn, _ in cases.values():
            for _ in range(10):
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
            out[f"{name}_{tag}"] = round(ms, 5)
            out[f"{name}_{tag}_range"] = round(max(times[name]) - min(times[name]), 5)
            out[f"{name}_{tag}_hbm_fraction"] = round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4)
        out[f"contrast_over_copy_hbm_fraction_{tag}"] = round(out[f"contrast_{tag}_hbm_fraction"] / out[f"copy_scene_{tag}_hbm_fraction"], 3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
