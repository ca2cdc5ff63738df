"""Timings of the motion-vectors pass (include/sah_motion_vectors.h) against the G-buffer pass of the same scene on cuda:0: the dense
atrium (23 808 triangles), the camera inside it, a moved last frame; 1920 x 1080 and 3840 x 2160.

    python tools/bench_motion_vectors.py [--calls 50] [--rounds 5]

Both calls end in a host synchronisation of their own (the rasteriser reads its counters back), so a call is timed on the host clock
around N back-to-back calls; the two passes alternate, round by round, and the median of the rounds is reported.  Prints one JSON line,
milliseconds per call."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, images, lib, mesh, scene

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(8).arrays()), keep)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    for (W, H, tag) in ((1920, 1080, "1080p"), (3840, 2160, "4k")):
        view = scene.SceneView()
        view.set_render_resolution(W, H)
        view.set_perspective_projection(75.0, W / H, 0.05)
        view.rotate(0.0, math.radians(90.0))
        view.set_position([0.0, 1.0, 0.0])
        view.jitter = np.array([0.3, -0.2], np.float32)
        view.update_transforms()
        view.rotate(0.02, 0.03)
        view.set_position([-0.3, 1.1, 0.2])
        view.jitter = np.array([-0.25, 0.4], np.float32)
        view.update_transforms()
        gb = {"color": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "normals": torch.zeros((H, W, 4), dtype=torch.int16, device="cuda"),
              "data": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "emission": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"),
              "depth": torch.zeros((H, W), dtype=torch.float32, device="cuda")}
        mv = torch.zeros((H, W, 2), dtype=torch.int16, device="cuda")
        G, D, M = images.gbuffer(gb), images.plane(gb["depth"], _abi.FORMAT_D32_SFLOAT), images.plane(mv, _abi.FORMAT_R16G16_SFLOAT)
        cases = {"gbuffer": lambda: ctx.gbuffer_render(geo, view.gpu_data, G), "motion_vectors": lambda: ctx.motion_vectors_render(geo, view.gpu_data, D, M)}
        times = {k: [] for k in cases}
        for fn in cases.values():
            for _ in range(10):
                fn()
        for _ in range(args.rounds):
            for name, fn in cases.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / args.calls)
        for name in cases:
            out[f"{name}_{tag}"] = round(statistics.median(times[name]), 5)
            out[f"{name}_{tag}_range"] = round(max(times[name]) - min(times[name]), 5)
        out[f"mv_over_gbuffer_{tag}"] = round(out[f"motion_vectors_{tag}"] / out[f"gbuffer_{tag}"], 3)
        out[f"solid_won_{tag}"] = round(float((gb["depth"] > 0).float().mean()), 4)
        out[f"written_{tag}"] = round(float((mv != 0).any(-1).float().mean()), 4)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
