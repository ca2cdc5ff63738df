"""Timings of sah_taa_upscale (include/sah_taa_upscale.h) on cuda:0 to 3840 x 2160 from 2560 x 1440 and from 1920 x 1080, with
sah_taa_resolve at 3840 x 2160 — what the same output costs without an upscaler — in the same process as the yardstick; and the figure the
upscaler exists for: sah_lighting (the headline workload of bench.py: atrium, CSM sun, LPV) at the render resolution plus the upscale, against
sah_lighting at 4K plus the resolve.

    python tools/bench_taa_upscale.py [--calls 50] [--rounds 7] [--no-lighting]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Both passes ping-pong two targets, as a caller does.  Prints one JSON
line: milliseconds per call, GB/s over the algorithmic bytes — per OUTPUT pixel 16 (history read, output written) + 16 w h / (W H) (lit 8 +
depth 4 + motion vectors 4 per render texel) for the upscale, 32 for the resolve — and that rate as a fraction of the 6.3 TB/s a copy kernel
achieves on this device."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ACHIEVABLE_BYTES_PER_S = 6.3e12
OUTPUT = (3840, 2160)
RENDERS = {"1440p": (2560, 1440), "1080p": (1920, 1080), "4k": OUTPUT}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-lighting", action="store_true", help="the two anti-aliasing passes alone")
    args = ap.parse_args()
    import torch

    from androidrenderer_amd import _abi, frame, images, lib

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    RGBA, D32, RG = _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16_SFLOAT
    W, H = OUTPUT
    g = torch.Generator(device="cuda").manual_seed(1)
    targets = [torch.randint(0, 0x4400, (H, W, 4), dtype=torch.int16, device="cuda", generator=g), torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")]
    T_ = [images.plane(t, RGBA) for t in targets]
    state = {"i": 0}
    planes, keep = {}, []
    for tag, (w, h) in RENDERS.items():
        lit = torch.randint(0, 0x4400, (h, w, 4), dtype=torch.int16, device="cuda", generator=g)  # finite halfs in [0, 4)
        depth = torch.rand((h, w), dtype=torch.float32, device="cuda", generator=g)
        mv = (torch.rand((h, w, 2), device="cuda", generator=g) * 2 - 1).to(torch.float16).view(torch.int16)  # within a pixel, as under a jitter
        keep.append((lit, depth, mv))
        planes[tag] = (images.plane(lit, RGBA), images.plane(depth, D32), images.plane(mv, RG))

    def upscale_params(flags):
        p = _abi.TaaUpscaleParams()
        p.blend, p.min_confidence, p.flags = 0.1, 0.05, flags
        p.jitter[:] = [0.25, -0.125]
        p.previous_jitter[:] = [-0.25, 0.375]
        return p

    def resolve_params(flags):
        p = _abi.TaaParams()
        p.blend, p.flags = 0.1, flags
        p.jitter[:] = [0.25, -0.125]
        p.previous_jitter[:] = [-0.25, 0.375]
        return p
    UP, RP = {f: upscale_params(f) for f in (0, 1, 2)}, {f: resolve_params(f) for f in (0, 2)}

    def upscale(tag, flags):
        i = state["i"]
        L_, D_, M_ = planes[tag]
        ctx.taa_upscale(L_, D_, M_, None if flags & 1 else T_[i], T_[1 - i], UP[flags])
        state["i"] = 1 - i

    def resolve(flags):
        i = state["i"]
        L_, D_, M_ = planes["4k"]
        ctx.taa_resolve(L_, D_, M_, T_[i], T_[1 - i], RP[flags])
        state["i"] = 1 - i

    def upscale_bytes(tag, history=True):
        w, h = RENDERS[tag]
        return (16 if history else 8) * W * H + 16 * w * h
    cases = {"upscale_1440p_to_4k": (lambda: upscale("1440p", 0), upscale_bytes("1440p")), "upscale_1440p_to_4k_hdr": (lambda: upscale("1440p", 2), upscale_bytes("1440p")),
             "upscale_1080p_to_4k": (lambda: upscale("1080p", 0), upscale_bytes("1080p")), "upscale_1080p_to_4k_hdr": (lambda: upscale("1080p", 2), upscale_bytes("1080p")),
             "upscale_1440p_to_4k_no_history": (lambda: upscale("1440p", 1), upscale_bytes("1440p", False)),
             "taa_4k": (lambda: resolve(0), 32 * W * H), "taa_4k_hdr": (lambda: resolve(2), 32 * W * H)}
    if not args.no_lighting:
        # the headline workload of bench.py at the two render resolutions, each followed by the pass that brings it to an antialiased 4K frame
        def lighting(tag):
            w, h = RENDERS[tag]
            fr = frame.LightingInputs(w, h, seed=2, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flavour="atrium", shadowmap_res=4096, synth_device="cuda")
            fr.lpv_generation = 1  # the library keeps its gather copy of the volumes
            dev = fr.device_arrays("cuda")
            lit = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
            desc, held = fr.describe(dev, lit)
            keep.append((fr, dev, lit, held))
            return desc, images.plane(lit, RGBA)
        (d1440, l1440), (d4k, l4k) = lighting("1440p"), lighting("4k")

        def frame_1440p():
            ctx.lighting(d1440)
            i = state["i"]
            ctx.taa_upscale(l1440, planes["1440p"][1], planes["1440p"][2], T_[i], T_[1 - i], UP[2])
            state["i"] = 1 - i

        def frame_4k():
            ctx.lighting(d4k)
            i = state["i"]
            ctx.taa_resolve(l4k, planes["4k"][1], planes["4k"][2], T_[i], T_[1 - i], RP[2])
            state["i"] = 1 - i
        cases.update({"lighting_1440p": (lambda: ctx.lighting(d1440), None), "lighting_4k": (lambda: ctx.lighting(d4k), None),
                      "lighting_1440p_plus_upscale_hdr": (frame_1440p, None), "lighting_4k_plus_taa_hdr": (frame_4k, None)})
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
        out[name] = round(ms, 5)
        out[f"{name}_range"] = round(max(times[name]) - min(times[name]), 5)
        if nbytes:
            out[f"{name}_gb_per_s"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
            out[f"{name}_of_achievable"] = round(nbytes / (ms * 1e-3) / ACHIEVABLE_BYTES_PER_S, 4)
    if not args.no_lighting:
        out["frame_1440p_upscaled_over_frame_4k"] = round(out["lighting_1440p_plus_upscale_hdr"] / out["lighting_4k_plus_taa_hdr"], 4)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
