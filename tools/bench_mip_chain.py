"""Timings of the mip-chain generator (include/sah_mip_chain.h) on cuda:0: the Hi-Z pyramid of a D32 depth buffer at 1280 x 720, 1920 x 1080 and
3840 x 2160 render resolution (level 0 and level count from DepthCullingPhase's formulas: resolution / 2, round(log2(major dimension))) and
the RGBA16F chain at 3840 x 2160, with sah_copy_scene at the same extent in the same process as the yardstick (16 B/px).  7680 x 4320 is not
run: the entry refuses a source above 4096 in either axis (SPD's 12 levels end there).

    python tools/bench_mip_chain.py [--calls 50] [--rounds 7]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Prints one JSON line: milliseconds per call, the HBM fraction by
algorithmic bytes over 8 TB/s — the source read once and every level written once — and the ratio of that fraction to the copy's."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
EXCLUDED = ["7680x4320: the source exceeds SAH_MIP_CHAIN_MAX_SOURCE (4096)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, images, lib

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0), "excluded": EXCLUDED}
    keep, cases = [], {}
    g = torch.Generator(device="cuda").manual_seed(1)

    def chain(tag, W, H, src_fmt, dst_fmt):
        bpp = _abi.FORMAT_BPP[dst_fmt]
        w0, h0 = W // 2, H // 2
        n = int(np.round(np.log2(np.float32(max(w0, h0)))))
        if src_fmt == _abi.FORMAT_D32_SFLOAT:
            src = torch.rand((H, W), dtype=torch.float32, device="cuda", generator=g)
            levels = [torch.zeros((max(1, h0 >> i), max(1, w0 >> i)), dtype=torch.float32, device="cuda") for i in range(n)]
        else:
            src = torch.randint(0, 0x3c00, (H, W, 4), dtype=torch.int16, device="cuda", generator=g)
            levels = [torch.zeros((max(1, h0 >> i), max(1, w0 >> i), 4), dtype=torch.int16, device="cuda") for i in range(n)]
        S_, L_ = images.plane(src, src_fmt), [images.plane(t, dst_fmt) for t in levels]
        keep.append((src, levels, S_, L_))
        nbytes = W * H * _abi.FORMAT_BPP[src_fmt] + sum(t.shape[0] * t.shape[1] * bpp for t in levels)
        cases[tag] = ((lambda: ctx.mip_chain_generate(S_, L_)), nbytes)

    def copy(tag, W, H):
        lit = torch.randint(0, 0x3c00, (H, W, 4), dtype=torch.int16, device="cuda", generator=g)
        aa = torch.zeros_like(lit)
        A_, B_ = images.plane(lit, _abi.FORMAT_R16G16B16A16_SFLOAT), images.plane(aa, _abi.FORMAT_R16G16B16A16_SFLOAT)
        keep.append((lit, aa, A_, B_))
        cases[tag] = ((lambda: ctx.copy_scene(A_, B_)), 16 * W * H)

    for W, H in ((1280, 720), (1920, 1080), (3840, 2160)):
        chain(f"hi_z_{W}x{H}", W, H, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R32_SFLOAT)
        copy(f"copy_scene_{W}x{H}", W, H)
    chain("rgba16f_3840x2160", 3840, 2160, _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R16G16B16A16_SFLOAT)
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
        out[f"{name}_hbm_fraction"] = round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4)
    for name in cases:
        if not name.startswith("copy_scene"):
            res = name.rsplit("_", 1)[1]
            out[f"{name}_over_copy_hbm_fraction"] = round(out[f"{name}_hbm_fraction"] / out[f"copy_scene_{res}_hbm_fraction"], 3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
