"""Timings of sah_gbuffer_motion_render (include/sah_gbuffer_motion.h) against the two calls it replaces — sah_gbuffer_render, then
sah_motion_vectors_render — on cuda:0: mesh.atrium(8) (23 808 triangles), the camera inside it, a moved last frame (the view of
tools/bench_motion_vectors.py); 1920 x 1080 and 3840 x 2160.

    python tools/bench_gbuffer_motion.py [--calls 20] [--rounds 7] [--out profiles/gbuffer_motion.txt]

Time    events around N back-to-back repetitions after a warm-up, the two cases alternating round by round in one process; the median of
        the rounds and the spread (largest minus smallest round).  Every call of either kind waits for the stream once per rasteriser
        pass (the read-back of the counters), so the figures are what a caller pays, host stalls included.
Equal   the six planes of the fused call against the two calls', byte for byte, at the timed sizes.
Accept  the fused call is faster than the two calls by more than the spread of the two-call figure.
Prints one JSON line and, with --out, writes the table."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, images, lib, mesh, scene

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(8).arrays()), keep)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per frame, median of the rounds", "device": torch.cuda.get_device_name(0), "triangles": 23808}
    lines = [f"sah_gbuffer_motion_render against sah_gbuffer_render + sah_motion_vectors_render: atrium(8), camera inside, {out['device']}",
             f"events around {args.calls} repetitions, {args.rounds} rounds, the cases alternating; ms per frame: median (spread = max - min of the rounds)", ""]

    def targets(W, H):
        t = {"color": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "normals": torch.zeros((H, W, 4), dtype=torch.int16, device="cuda"),
             "data": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "emission": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"),
             "depth": torch.zeros((H, W), dtype=torch.float32, device="cuda"), "motion_vectors": torch.full((H, W, 2), 0x5A5A, dtype=torch.int16, device="cuda")}
        return t, images.gbuffer(t), images.plane(t["depth"], _abi.FORMAT_D32_SFLOAT), images.plane(t["motion_vectors"], _abi.FORMAT_R16G16_SFLOAT)

    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
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
        vd = view.gpu_data
        (t2, G2, D2, M2), (tf, Gf, _, Mf) = targets(W, H), targets(W, H)

        def two_calls():
            ctx.gbuffer_render(geo, vd, G2)
            ctx.motion_vectors_render(geo, vd, D2, M2)

        def fused():
            ctx.gbuffer_motion_render(geo, vd, Gf, Mf)

        cases = {"two_calls": two_calls, "fused": fused}
        for fn in cases.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        equal = all(torch.equal(t2[k], tf[k]) if k != "depth" else torch.equal(t2[k].view(torch.int32), tf[k].view(torch.int32)) for k in t2)
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for name, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.calls)
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        saved = med["two_calls"] - med["fused"]
        accepted = saved > spread["two_calls"]
        tag = f"{W}x{H}"
        out[tag] = {"two_calls": round(med["two_calls"], 5), "two_calls_spread": round(spread["two_calls"], 5), "fused": round(med["fused"], 5),
                    "fused_spread": round(spread["fused"], 5), "saved": round(saved, 5), "outputs_equal": equal, "accepted": bool(accepted),
                    "moving_texels": round(float((tf["motion_vectors"] != 0).any(-1).float().mean()), 3)}
        lines += [f"{tag}:  two calls {med['two_calls']:.4f} ({spread['two_calls']:.4f})   fused {med['fused']:.4f} ({spread['fused']:.4f})   saved {saved:.4f} ms "
                  f"= {100.0 * saved / med['two_calls']:.1f} % of the two calls",
                  f"{' ' * len(tag)}   rounds, two calls: {' '.join(f'{v:.4f}' for v in times['two_calls'])}",
                  f"{' ' * len(tag)}   rounds, fused:     {' '.join(f'{v:.4f}' for v in times['fused'])}",
                  f"{' ' * len(tag)}   six planes byte-equal: {equal};  texels with a motion vector: {out[tag]['moving_texels']};  "
                  f"faster by more than the two-call spread: {bool(accepted)}", ""]
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
