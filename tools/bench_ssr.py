"""Timings of sah_ssr (include/sah_ssr.h) on cuda:0 at 3840 x 2160 with the header's default parameters, on two scenes: the rasterised
atrium and the analytic mirror room of tests/ssr_ref.py (a metal floor under a wall).  The lit image is random HDR noise on the atrium (the
pass's time depends on the geometry, not on the colours) and the room's own on the room; the reflections are taken from the lit image
itself.  With --compare, sah_ssao (two blur passes) and sah_taa_resolve (with a history) on the atrium's planes in the same process: the
two image-space passes to read the times against.

    python tools/bench_ssr.py [--calls 30] [--rounds 7] [--compare]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Prints one JSON line.  SAH_HIP_LIBRARY selects another build of the
library (androidrenderer_amd/lib.py).  That is how profiles/ssr.txt compared the march with and without the block skip: the skip lived in
ssr.hip then, and a second library was built from a patched copy without it.  Neither form of the skip is in the tree any more (it lost,
and the rule was that no variant stays in the source), so that comparison cannot be repeated from this tree: DESIGN.md section 5w
describes the skip closely enough to write it again."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 3840, 2160


def measure(args):
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, frame, lib, mesh, scene
    from tests import ssr_ref

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"library": os.path.basename(lib.LIB_PATH), "extent": [W, H], "calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds",
           "device": torch.cuda.get_device_name(0)}
    keep, cases = [], {}

    def ssr_case(name, gb, lit, view_data):
        reflections = frame.ScreenSpaceReflections(ctx, W, H)
        keep.append((gb, lit, view_data, reflections))
        cases[name] = lambda: reflections(view_data, gb, lit)
        res = reflections(view_data, gb, lit)
        torch.cuda.synchronize()
        out[f"{name}_changed"] = round(float((res[..., :3] != lit[..., :3]).any(-1).float().mean()), 4)

    # the rasterised atrium
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    view = scene.SceneView.default(W, H)
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    gb = {k: torch.zeros((H, W) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
    mv = torch.zeros((H, W, 2), dtype=torch.int16, device="cuda")
    frame.rasterised_frame(ctx, geo, view.gpu_data, gb, motion_vectors=mv)
    torch.cuda.synchronize()
    out["atrium_covered"] = round(float((gb["depth"] > 0).float().mean()), 3)
    lit = (torch.rand((H, W, 4), device="cuda") * 2).to(torch.float16).view(torch.int16)
    ssr_case("ssr_atrium", gb, lit, view.gpu_data)
    # the mirror room
    room = ssr_ref.mirror_room(W, H)[0]
    room_gb = {k: frame.to_torch(np.ascontiguousarray(room[k])) for k in ("color", "normals", "data", "depth")}
    room_view = _abi.ViewData()
    rv = ssr_ref.room_view()
    for i in range(16):
        room_view.view[i] = float(rv.view[i])
    room_view.projection[0], room_view.projection[5], room_view.projection[8], room_view.projection[9] = float(rv.p00), float(rv.p11), float(rv.p20), float(rv.p21)
    room_view.projection[11], room_view.z_near = -1.0, float(rv.z_near)
    ssr_case("ssr_room", room_gb, frame.to_torch(np.ascontiguousarray(room["lit"])), room_view)
    if args.compare:
        ao = frame.ScreenSpaceAO(ctx, W, H)
        taa = frame.TemporalResolver(ctx, W, H)
        taa.resolve(lit, gb["depth"], mv, (0.25, -0.25))
        cases["ssao_atrium_blur2"] = lambda: ao.generate(view.gpu_data, gb["depth"], gb["normals"])
        cases["taa_resolve_atrium"] = lambda: taa.resolve(lit, gb["depth"], mv, (0.25, -0.25))
    times = {k: [] for k in cases}
    for fn in cases.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
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
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--compare", action="store_true")
    measure(ap.parse_args())


if __name__ == "__main__":
    main()
