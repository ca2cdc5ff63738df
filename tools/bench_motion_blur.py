"""Timings of sah_motion_blur (include/sah_motion_blur.h) on cuda:0 with the header's default parameters, at 3840 x 2160 and at
2560 x 1440 -> 3840 x 2160, over three vector fields: a static camera (every pixel passes through: the pass is a copy plus the tile
reduction), a pan in which every tile blurs (one vector for the whole frame, 24 pixels), and a pan of the rasterised atrium (the camera turned
between two frames, the vectors from sah_motion_vectors_render, the depth the rasteriser's).  The scene is random HDR noise: the pass's time
depends on the vectors and the depth, not on the colours.  In the same process, on the same planes: sah_taa_resolve (with a history) and
sah_exposure_apply, the two passes to read the times against — the second moves the 16 B/px a static frame moves, less its 4 B/px of vectors.

    python tools/bench_motion_blur.py [--calls 30] [--rounds 7]

No call synchronises with the host, so a case is timed with events around N back-to-back calls after a warm-up; the cases alternate round
by round, and the median of the rounds is reported with the range.  Prints one JSON line.  SAH_HIP_LIBRARY selects another build of the
library (androidrenderer_amd/lib.py)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 3840, 2160
LOW = (2560, 1440)


def measure(args):
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, frame, images, lib, mesh, scene

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"library": os.path.basename(lib.LIB_PATH), "output": [W, H], "low": list(LOW), "calls": args.calls, "rounds": args.rounds,
           "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    keep, cases = [], {}
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    scene_t = (torch.rand((H, W, 4), device="cuda") * 2).to(torch.float16).view(torch.int16)
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}

    def atrium(w, h):
        """depth and motion vectors of the atrium, the camera turned by 2 degrees since the last frame"""
        view = scene.SceneView.default(w, h)
        view.rotate(0.0, math.radians(2.0))
        view.update_transforms()
        gb = {k: torch.zeros((h, w) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
        mv = torch.zeros((h, w, 2), dtype=torch.int16, device="cuda")
        frame.rasterised_frame(ctx, geo, view.gpu_data, gb, motion_vectors=mv)
        torch.cuda.synchronize()
        return gb["depth"], mv, view.near_value

    def constant(w, h, vector):
        return torch.from_numpy(np.broadcast_to(np.array(vector, np.float16), (h, w, 2)).copy().view(np.int16)).cuda()

    for tag, (w, h) in (("4k", (W, H)), ("1440p_to_4k", LOW)):
        depth, mv_atrium, z_near = atrium(w, h)
        out[f"{tag}_atrium_covered"] = round(float((depth > 0).float().mean()), 3)
        for name, mv in (("static", constant(w, h, (0.0, 0.0))), ("pan_all", constant(w, h, (24.0, 7.0))), ("pan_atrium", mv_atrium)):
            blur = frame.MotionBlur(ctx, W, H, w, h, z_near=z_near)
            keep.append((blur, depth, mv))
            cases[f"{tag}_{name}"] = lambda blur=blur, depth=depth, mv=mv: blur(scene_t, depth, mv)
            res = blur(scene_t, depth, mv)
            torch.cuda.synchronize()
            out[f"{tag}_{name}_changed"] = round(float((res != scene_t).any(-1).float().mean()), 4)
        if tag == "4k":
            taa = frame.TemporalResolver(ctx, W, H)
            taa.resolve(scene_t, depth, mv_atrium, (0.25, -0.25))
            cases["taa_resolve_4k"] = lambda taa=taa, depth=depth, mv=mv_atrium: taa.resolve(scene_t, depth, mv, (0.25, -0.25))
    state = torch.from_numpy(np.frombuffer(np.array([1.5, 1.5], np.float32).tobytes() + np.array([1, 0], np.uint32).tobytes(), np.uint8).copy()).cuda()
    exposed = torch.zeros_like(scene_t)
    rgba16 = _abi.FORMAT_R16G16B16A16_SFLOAT
    cases["exposure_apply_4k"] = lambda: ctx.exposure_apply(images.plane(scene_t, rgba16), state.data_ptr(), images.plane(exposed, rgba16))
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
    out["static_over_exposure_apply"] = round(out["4k_static"] / out["exposure_apply_4k"], 3)
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    measure(ap.parse_args())


if __name__ == "__main__":
    main()
