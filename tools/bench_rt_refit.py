"""Timings of sah_rt_refit (include/sah_rt_refit.h) against sah_rt_build on cuda:0, and what the stale order of a refit structure costs the
rays, on mesh.atrium(8) (23 808 triangles) and on the 3000-primitive scene of the structure tests (4439 triangles).

    python tools/bench_rt_refit.py [--calls 20] [--rounds 7]

Time    events around N back-to-back calls after a warm-up, cases alternating round by round, the median of the rounds with the range.
        sah_rt_build waits for the stream twice per call, so its figure is what a caller pays per build, host stalls included; the refit
        never meets the host.  The build's kernels are the same in this tree as before the refit existed (rt.hip's build kernels are untouched).
Stale   every box of the atrium moved by a random offset of up to 1 m per axis: sah_rtao and sah_sun_shadow_mask at 1920 x 1080 through
order   the structure built on the unmoved atrium and refit, against a structure built on the moved one; and rt_structure_ref.tree_cost
        (sum of node areas / root area) of both orders.  The two structures give the same planes (checked).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, images, lib, mesh, scene, synth
    from tests import rt_structure_ref as ref
    from tests import rt_structure_scenes as scenes

    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    keep = []

    def context():
        c = lib.Context(0)
        c.set_stream(stream)
        return c

    def device_geo(arrays):
        return mesh.geometry(mesh.to_device(arrays), keep)

    def timed(cases):
        times = {k: [] for k in cases}
        for fn in cases.values():
            for _ in range(3):
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

    # ---- build against refit
    atrium = mesh.atrium(8)
    moved = mesh.atrium(8)
    g = synth.rng(8)
    for p in moved.primitives:
        model = np.eye(4, dtype=np.float32)
        model[:3, 3] = g.uniform(-1.0, 1.0, 3)
        p["model"] = model.T.reshape(16)
    ctx = context()
    for tag, m in (("atrium8", atrium), ("primitives3000", scenes.many_primitives(3000))):
        geo = device_geo(m.arrays())
        stats = ctx.rt_build(geo)
        out[f"{tag}_triangles"], out[f"{tag}_levels"] = stats[0], stats[2]
        timed({f"{tag}_rt_build": (lambda geo=geo: ctx.rt_build(geo)), f"{tag}_rt_refit": (lambda geo=geo: ctx.rt_refit(geo))})
        out[f"{tag}_build_over_refit"] = round(out[f"{tag}_rt_build"] / out[f"{tag}_rt_refit"], 2)

    # ---- the stale order: built on the atrium and refit to the moved one, against built on the moved one
    W, H = 1920, 1080
    view = scene.SceneView.default(W, H)
    sun = scene.DirectionalLight(shadow_mode=_abi.SHADOW_MODE_RT, num_shadow_samples=4.0)
    moved_geo = device_geo(moved.arrays())
    gb = {"color": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "normals": torch.zeros((H, W, 4), dtype=torch.int16, device="cuda"),
          "data": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"), "emission": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"),
          "depth": torch.zeros((H, W), dtype=torch.float32, device="cuda")}
    ctx.gbuffer_render(moved_geo, view.gpu_data, images.gbuffer(gb))
    noise = torch.from_numpy(synth.rng(2).integers(0, 256, (128, 128, 4), dtype=np.uint8)).cuda()
    d, n, z = images.plane(gb["depth"], _abi.FORMAT_D32_SFLOAT), images.plane(gb["normals"], _abi.FORMAT_R16G16B16A16_SFLOAT), images.plane(noise, _abi.FORMAT_R8G8B8A8_UNORM)
    planes = {}
    contexts = {"refit": ctx, "rebuilt": context()}
    ctx.rt_build(device_geo(atrium.arrays()))
    ctx.rt_refit(moved_geo)
    contexts["rebuilt"].rt_build(moved_geo)
    cases = {}
    for tag, c in contexts.items():
        out[f"atrium8_moved_tree_cost_{tag}"] = round(ref.tree_cost(c.rt_structure()["tris"]), 4)
        ao, mask = (torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in range(2))
        planes[tag] = (ao, mask)
        a_, m_ = images.plane(ao, _abi.FORMAT_R32_SFLOAT), images.plane(mask, _abi.FORMAT_R32_SFLOAT)
        keep.append((a_, m_))
        cases[f"rtao_1080p_{tag}"] = (lambda c=c, a_=a_: c.rtao(view.gpu_data, d, n, z, 1, 8.0, a_))
        cases[f"shadow_mask_1080p_{tag}"] = (lambda c=c, m_=m_: c.sun_shadow_mask(view.gpu_data, sun.constants, d, n, z, m_))
    timed(cases)
    torch.cuda.synchronize()
    out["planes_equal"] = all(torch.equal(planes["refit"][i].view(torch.int32), planes["rebuilt"][i].view(torch.int32)) for i in range(2))
    out["covered"] = round(float((gb["depth"] > 0).float().mean()), 3)
    for k in ("rtao", "shadow_mask"):
        out[f"{k}_1080p_refit_over_rebuilt"] = round(out[f"{k}_1080p_refit"] / out[f"{k}_1080p_rebuilt"], 3)
    for c in contexts.values():
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
