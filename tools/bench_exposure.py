"""Timings of sah_exposure_meter and sah_exposure_apply (include/sah_exposure.h) on cuda:0 at 1280 x 720, 2560 x 1440 and 3840 x 2160 on a
log-normal image 2.5 octaves wide: the metering alone, apply alone, and the fused call; at each extent also the metering alone on a CONSTANT
image — every lane of every wave on one bin of its LDS sub-histogram — against the log-normal one; and sah_taa_resolve at the same extents
in the same process, which reads and writes comparable planes.

    python tools/bench_exposure.py [--calls 30] [--rounds 7]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Prints one JSON line: milliseconds per call, GB/s over the algorithmic
bytes — 8 B/px read, + 8 B/px written with the store — and that rate as a fraction of the 6.3 TB/s a copy kernel achieves on this device
(DESIGN.md §7)."""
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
    import torch

    from androidrenderer_amd import _abi, images, lib

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT
    keep, cases = [], {}
    g = torch.Generator(device="cuda").manual_seed(5)
    for tag, (w, h) in EXTENTS.items():
        lum = 0.2 * torch.exp2(2.5 * torch.randn((h, w, 1), device="cuda", generator=g))
        wide = torch.cat([lum * (0.3 + 1.4 * torch.rand((h, w, 3), device="cuda", generator=g)), torch.ones((h, w, 1), device="cuda")], -1).to(torch.float16)
        flat = torch.full((h, w, 4), 0.25, device="cuda", dtype=torch.float16)
        exposed = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
        work = torch.zeros(260, dtype=torch.int32, device="cuda")
        states = torch.zeros((2, 4), dtype=torch.float32, device="cuda")
        states[0, 0] = 0.5
        depth = torch.rand((h, w), dtype=torch.float32, device="cuda")
        mv = torch.zeros((h, w, 2), dtype=torch.float16, device="cuda")
        history = wide.clone()
        keep.append((wide, flat, exposed, work, states, depth, mv, history))
        wide_p, flat_p, out_p = images.plane(wide, RGBA16F), images.plane(flat, RGBA16F), images.plane(exposed, RGBA16F)
        s0, s1, wk = states[0].data_ptr(), states[1].data_ptr(), work.data_ptr()
        params = _abi.ExposureParams.default()
        taa = _abi.TaaParams()
        taa.blend, taa.flags = 0.1, _abi.TAA_HDR_WEIGHTS
        depth_p, mv_p, hist_p = images.plane(depth, _abi.FORMAT_D32_SFLOAT), images.plane(mv, _abi.FORMAT_R16G16_SFLOAT), images.plane(history, RGBA16F)
        cases[f"meter_{tag}"] = (lambda wide_p=wide_p, s0=s0, s1=s1, wk=wk, params=params: ctx.exposure_meter(wide_p, s0, s1, wk, None, params), 8 * w * h)
        cases[f"meter_constant_{tag}"] = (lambda flat_p=flat_p, s0=s0, s1=s1, wk=wk, params=params: ctx.exposure_meter(flat_p, s0, s1, wk, None, params), 8 * w * h)
        cases[f"apply_{tag}"] = (lambda wide_p=wide_p, s0=s0, out_p=out_p: ctx.exposure_apply(wide_p, s0, out_p), 16 * w * h)
        cases[f"fused_{tag}"] = (lambda wide_p=wide_p, s0=s0, s1=s1, wk=wk, out_p=out_p, params=params: ctx.exposure_meter(wide_p, s0, s1, wk, out_p, params), 16 * w * h)
        cases[f"taa_resolve_{tag}"] = (lambda wide_p=wide_p, depth_p=depth_p, mv_p=mv_p, hist_p=hist_p, out_p=out_p, taa=taa:
                                       ctx.taa_resolve(wide_p, depth_p, mv_p, hist_p, out_p, taa), None)
        cases[f"meter_{tag}"][0]()
        torch.cuda.synchronize()
        n = work[:256].cpu().numpy()
        out[f"{tag}_bins_in_use"] = int((n != 0).sum())
        out[f"{tag}_largest_bin_share"] = round(float(n.max()) / float(max(n.sum(), 1)), 4)
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
        out[f"constant_over_lognormal_{tag}"] = round(out[f"meter_constant_{tag}"] / out[f"meter_{tag}"], 3)
        out[f"fused_over_taa_resolve_{tag}"] = round(out[f"fused_{tag}"] / out[f"taa_resolve_{tag}"], 3)
        out[f"fused_over_meter_plus_apply_{tag}"] = round(out[f"fused_{tag}"] / (out[f"meter_{tag}"] + out[f"apply_{tag}"]), 3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
