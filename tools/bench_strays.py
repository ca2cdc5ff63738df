"""Times sah_lighting (CSM sun + LPV, the headline's kernel) over a frame or a band of its rows with the fast kernel's strays finished as
asked — by the context's record of recent calls, always by the fix-up launch, or always in the fast kernel (lib.Context.debug_set's
`strays`) — on one GPU, HIP events on the launch stream.  Prints one JSON line: ms per call, the listed pixels, and which form the
call before the timed ones and the last of them took.  For the price of a wrong prediction (a frame full of strays finished in-kernel) and for launches too small for
bench.py's workloads (one rank's band of the 4K frame).

    python tools/bench_strays.py [--width 3840 --height 2160] [--flavour atrium|random] [--rows 945 1215] [--strays auto|launch|inline] [--iters 400]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--flavour", choices=["atrium", "random"], default="atrium")
    ap.add_argument("--rows", type=int, nargs=2, default=(0, 0), metavar=("BEGIN", "END"))
    ap.add_argument("--strays", choices=["auto", "launch", "inline"], default="auto")
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--ramp-ms", type=float, default=200.0, help="untimed: the call runs back to back for this long first (the clock ramp bench.py gives its step)")
    args = ap.parse_args()
    import torch

    from androidrenderer_amd import _abi, frame, lib

    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    f = frame.LightingInputs(args.width, args.height, seed=2, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flavour=args.flavour, shadowmap_res=4096,
                             synth_device="cuda")
    f.row_begin, f.row_end = args.rows
    dev = f.device_arrays()
    lit = torch.zeros((args.height, args.width, 4), dtype=torch.int16, device="cuda")
    d, keep = f.describe(dev, lit)
    ctx.debug_set(strays=args.strays)
    t_end = time.perf_counter() + args.ramp_ms * 1e-3
    while True:
        for _ in range(8):
            ctx.lighting(d)
        torch.cuda.synchronize()
        if time.perf_counter() >= t_end:
            break
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    first = ctx.lighting_dispatch()["strays"]  # (of the last ramp call; read outside the timed calls: the report may wait for the stream)
    e0.record()
    for _ in range(args.iters):
        ctx.lighting(d)
    e1.record()
    torch.cuda.synchronize()
    rep = ctx.lighting_dispatch()
    print(json.dumps({"library": os.path.basename(lib.LIB_PATH), "width": args.width, "height": args.height, "rows": list(args.rows), "flavour": args.flavour,
                      "strays_asked": args.strays, "strays_taken": [first, rep["strays"]], "ppt": rep["ppt"], "listed_pixels": ctx.deferred_pixels(),
                      "ms_per_call": round(e0.elapsed_time(e1) / args.iters, 5), "iters": args.iters}))
    ctx.close()


if __name__ == "__main__":
    main()
