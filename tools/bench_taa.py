"""Timings of sah_taa_resolve (include/sah_taa.h) on cuda:0 at 1920 x 1080 and 3840 x 2160, with sah_copy_scene — the pass it replaces — at
the same extent in the same process as the yardstick.

    python tools/bench_taa.py [--calls 50] [--rounds 7]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  The resolve ping-pongs two targets, as a caller does.  Prints one JSON
line: milliseconds per call, GB/s over the algorithmic bytes — 32 B/px for the resolve (lit 8 + depth 4 + motion vectors 4 + history 8 read,
8 written), 16 B/px for the copy and for the resolve without a history — and that rate as a fraction of the 6.3 TB/s a copy kernel achieves
on this device."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ACHIEVABLE_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    from androidrenderer_amd import _abi, images, lib

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    RGBA, D32, RG = _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16_SFLOAT
    for (W, H, tag) in ((1920, 1080, "1080p"), (3840, 2160, "4k")):
        g = torch.Generator(device="cuda").manual_seed(1)
        lit = torch.randint(0, 0x4400, (H, W, 4), dtype=torch.int16, device="cuda", generator=g)  # finite halfs in [0, 4)
        depth = torch.rand((H, W), dtype=torch.float32, device="cuda", generator=g)
        mv = (torch.rand((H, W, 2), device="cuda", generator=g) * 2 - 1).to(torch.float16).view(torch.int16)  # within a pixel, as under a jitter
        targets = [lit.clone(), torch.zeros_like(lit)]
        aa = torch.zeros_like(lit)
        L_, D_, M_, A_ = images.plane(lit, RGBA), images.plane(depth, D32), images.plane(mv, RG), images.plane(aa, RGBA)
        T_ = [images.plane(t, RGBA) for t in targets]
        state = {"i": 0}

        def params(flags):
            p = _abi.TaaParams()
            p.blend, p.flags = 0.1, flags
            p.jitter[:] = [0.25, -0.125]
            p.previous_jitter[:] = [-0.25, 0.375]
            return p
        P = {f: params(f) for f in (0, 1, 2)}

        def resolve(flags):
            i = state["i"]
            ctx.taa_resolve(L_, D_, M_, None if flags & 1 else T_[i], T_[1 - i], P[flags])
            state["i"] = 1 - i
        cases = {"taa": (lambda: resolve(0), 32 * W * H), "taa_hdr": (lambda: resolve(2), 32 * W * H), "taa_no_history": (lambda: resolve(1), 16 * W * H),
                 "copy_scene": (lambda: ctx.copy_scene(L_, A_), 16 * W * H)}
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
            out[f"{name}_{tag}_gb_per_s"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
            out[f"{name}_{tag}_of_achievable"] = round(nbytes / (ms * 1e-3) / ACHIEVABLE_BYTES_PER_S, 4)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
