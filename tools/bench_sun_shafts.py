"""Timings of sah_sun_shafts (include/sah_sun_shafts.h) on cuda:0 at 3840 x 2160 with 32 steps of half a unit, dithered, on the frame
bench.py's headline shades: the synthetic atrium G-buffer, its sun and four D16 cascades of 4096 x 4096 holding the atrium's own depth as
seen from the sun.  Downscale 1 (one fused launch) and downscale 2 (march at 1920 x 1080, then the depth-aware composite), and the same
two without a shadow map (the loop without its taps).  In the same process, on the same frame: sah_lighting with the CSM sun alone and
sah_ssr, the two passes to read the times against.

    python tools/bench_sun_shafts.py [--calls 20] [--rounds 7]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  The shadow taps per second divide the taps the numpy restatement counts
on every eighth pixel of every eighth row (scaled by 64: an estimate of the frame's) by the time.  Prints one JSON line.  SAH_HIP_LIBRARY
selects another build of the library (androidrenderer_amd/lib.py)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 3840, 2160
SHADOWMAP = 4096


def measure(args):
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, frame, lib
    from tests import sun_shafts_ref as ref

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"library": os.path.basename(lib.LIB_PATH), "extent": [W, H], "shadowmap": [SHADOWMAP, SHADOWMAP, 4], "calls": args.calls, "rounds": args.rounds,
           "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    fr = frame.LightingInputs(W, H, seed=2, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_NONE, sky=False, flavour="atrium", shadowmap_res=SHADOWMAP,
                              synth_device="cuda", shadow="scene")
    dev = fr.device_arrays()
    lit = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
    desc, keep = fr.describe(dev, lit)
    ctx.lighting(desc)
    torch.cuda.synchronize()
    view, sun = fr.view.gpu_data, fr.sun.constants
    settings = dict(flags=_abi.SUN_SHAFTS_DITHER, ambient=(2e-6, 3e-6, 5e-6))
    cases, passes = {}, {}
    for tag, shadow in (("", dev["shadowmap"]), ("_no_map", None)):
        for s in (1, 2):
            p = frame.SunShafts(ctx, W, H, downscale=s, **settings)
            passes[f"s{s}{tag}"] = p
            cases[f"sun_shafts_s{s}{tag}"] = lambda p=p, shadow=shadow: p(view, sun, shadow, dev["depth"], lit)
    cases["lighting_csm"] = lambda: ctx.lighting(desc)
    ssr = frame.ScreenSpaceReflections(ctx, W, H)
    cases["ssr"] = lambda: ssr(view, dev, lit)
    times = {k: [] for k in cases}
    for fn in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = passes["s1"](view, sun, dev["shadowmap"], dev["depth"], lit)
    out["s1_changed"] = round(float((res != lit).any(-1).float().mean()), 4)
    for _ in range(args.rounds):
        for name, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.calls)
    for name in cases:
        out[name] = round(statistics.median(times[name]), 5)
        out[f"{name}_range"] = round(max(times[name]) - min(times[name]), 5)
    # the taps of the frame, estimated by the restatement on a 1 / 64 subsample (the view's mapping depends on relative positions only)
    depth_small = dev["depth"][::8, ::8].cpu().numpy()
    small = ref.march(view, sun, dev["shadowmap"].cpu().numpy().view(np.uint16), depth_small, step_transmittance=float(passes["s1"].params.step_transmittance),
                      flags=ref.DITHER)
    out["samples_per_texel"] = round(small["samples"] / depth_small.size, 2)
    out["taps_per_texel"] = round(small["taps"] / depth_small.size, 2)
    for s in (1, 2):
        texels = ((W + s - 1) // s) * ((H + s - 1) // s)
        out[f"s{s}_gtaps_per_s"] = round(4 * out["taps_per_texel"] * texels / (out[f"sun_shafts_s{s}"] * 1e-3) / 1e9, 2)  # four texel reads a sample
    out["s2_over_s1"] = round(out["sun_shafts_s2"] / out["sun_shafts_s1"], 3)
    out["s1_over_lighting_csm"] = round(out["sun_shafts_s1"] / out["lighting_csm"], 3)
    del keep
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    measure(ap.parse_args())


if __name__ == "__main__":
    main()
