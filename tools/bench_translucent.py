"""Timings of sah_translucent_render (include/sah_translucent.h) on cuda:0 at 3840 x 2160, sun through the cascades + LPV + sky, over the
rasterised G-buffer of the atrium's opaque half (mesh.atrium(2, translucent_fraction=0.1)).  Three workloads:

    one_layer    one full-screen pane at alpha 0.5 (two triangles)
    four_layers  four such panes one behind the other
    atrium       the atrium's glass boxes (a tenth of its boxes), sorted back to front

Each is read against the opaque path's cost for the same triangles: sah_gbuffer_render of them as CUTOUT into a scratch G-buffer plus one
sah_lighting in the same sun / GI mode — what one layer of them costs where blending is not needed.  `*_per_layer_over_opaque` is the time of
the translucent call per layer of its deepest pixel (statistics word 7) over that cost.  Where the time goes: `*_alpha0` is the same workload
with every fragment's alpha code 0 — the set-up, the bins, every walk of the peel and the fragment texel, but no shading and no blend; the
difference to the real call is what lighting and blending the fragments cost.

    python tools/bench_translucent.py [--calls 10] [--rounds 7]

Every call ends with the rasteriser's read-back of its counters, a host synchronisation, so a case is timed with the host clock around N calls;
the cases alternate round by round, and the median of the rounds is reported with the range.  Prints one JSON line.  SAH_HIP_LIBRARY selects
another build of the library (androidrenderer_amd/lib.py)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 3840, 2160


def panes(m, count, alpha):
    """`count` full-screen panes, farthest first, 4 m and more in front of the camera of scene.SceneView.default"""
    from androidrenderer_amd import _abi, mesh
    for k in range(count):
        x = -3.0 + 0.5 * (count - 1 - k)
        mat = m.add_material(mesh.material(base=(0.4 + 0.1 * k, 0.8 - 0.1 * k, 0.9, alpha), rough=0.3, emission=(0.05, 0.05, 0.1, 0.0)))
        pos = [(x, -8.0, -12.0), (x, -8.0, 12.0), (x, 10.0, 12.0), (x, 10.0, -12.0)]
        m.add_primitive(pos, [(-1, 0, 0)] * 4, (0, 1, 2, 0, 2, 3), mat, ptype=_abi.PRIMITIVE_TYPE_TRANSLUCENT)


def measure(args):
    import numpy as np
    import torch

    from androidrenderer_amd import _abi, frame, images, lib, mesh

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"library": os.path.basename(lib.LIB_PATH), "extent": [W, H], "calls": args.calls, "rounds": args.rounds, "sun": "csm", "gi": "lpv",
           "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0)}
    fr = frame.LightingInputs(W, H, seed=2, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, sky=True, flavour="atrium", shadowmap_res=2048, synth_device="cuda")
    dev = fr.device_arrays()
    view = fr.view.gpu_data

    def device_scene(arrays):
        keep = []
        return mesh.geometry(mesh.to_device(arrays), keep), keep

    # the opaque frame: the atrium without its glass, rasterised, then lit
    atrium = mesh.atrium(2, translucent_fraction=0.1).arrays()
    opaque, glass = mesh.split_translucent(atrium)
    glass = mesh.sort_back_to_front(glass, view.view[:])
    geo_opaque, keep_o = device_scene(opaque)
    gb = {k: dev[k] for k in ("color", "normals", "data", "emission", "depth")}
    ctx.gbuffer_render(geo_opaque, view, images.gbuffer(gb))
    lit0 = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
    lit = torch.zeros_like(lit0)
    d0, keep0 = fr.describe(dev, lit0)
    ctx.lighting(d0)
    desc, keep1 = fr.describe(dev, lit)
    scratch = {k: torch.zeros_like(v) for k, v in gb.items()}
    scratch_lit = torch.zeros_like(lit0)
    dev_scratch = dict(dev)
    dev_scratch.update(scratch)
    d_scratch, keep2 = fr.describe(dev_scratch, scratch_lit)
    torch.cuda.synchronize()
    out["opaque_covered"] = round(float((dev["depth"] > 0).float().mean()), 4)

    def workload(arrays):
        """(translucent scene, the same with alpha code 0, the same as CUTOUT) on the device"""
        zero = dict(arrays, materials=arrays["materials"].copy())
        zero["materials"]["base_color_tint"][:, 3] = 0.0
        cut = dict(arrays, primitives=arrays["primitives"].copy(), materials=arrays["materials"].copy())
        cut["primitives"]["type"] = _abi.PRIMITIVE_TYPE_CUTOUT
        cut["materials"]["opacity_threshold"] = -1.0
        return device_scene(arrays), device_scene(zero), device_scene(cut)

    loads = {}
    for name, count in (("one_layer", 1), ("four_layers", 4)):
        m = mesh.Mesh()
        panes(m, count, 0.5)
        loads[name] = workload(m.arrays())
    loads["atrium"] = workload(glass)
    stats = torch.zeros(_abi.RASTER_STATS_WORDS, dtype=torch.int32, device="cuda")
    cases = {}
    for name, ((geo, _), (geo_zero, _), (geo_cut, _)) in loads.items():
        cases[name] = lambda geo=geo: ctx.translucent_render(desc, geo, stats.data_ptr())
        cases[f"{name}_alpha0"] = lambda geo=geo_zero: ctx.translucent_render(desc, geo)
        cases[f"{name}_gbuffer_as_cutout"] = lambda geo=geo_cut: ctx.gbuffer_render(geo, view, images.gbuffer(scratch))
    cases["lighting"] = lambda: (ctx.lighting(d_scratch), torch.cuda.synchronize())
    # what a call does to the image and how deep it goes, from a fresh lit image
    for name in loads:
        lit.copy_(lit0)
        cases[name]()
        torch.cuda.synchronize()
        s = stats.cpu().numpy().astype(np.uint32)
        out[f"{name}_triangles"], out[f"{name}_bin_entries"], out[f"{name}_deepest_pixel"] = int(s[3]), int(s[4]), int(s[7])
        out[f"{name}_changed"] = round(float((lit != lit0).any(-1).float().mean()), 4)
    for fn in cases.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(args.rounds):
        for name, fn in cases.items():
            lit.copy_(lit0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.calls)
    for name in cases:
        out[name] = round(statistics.median(times[name]), 4)
        out[f"{name}_range"] = round(max(times[name]) - min(times[name]), 4)
    for name in loads:
        layer = out[f"{name}_gbuffer_as_cutout"] + out["lighting"]
        out[f"{name}_opaque_path"] = round(layer, 4)
        out[f"{name}_per_layer_over_opaque"] = round(out[name] / max(1, out[f"{name}_deepest_pixel"]) / layer, 3)
        out[f"{name}_shade_and_blend"] = round(out[name] - out[f"{name}_alpha0"], 4)
    del keep_o, keep0, keep1, keep2
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    measure(ap.parse_args())


if __name__ == "__main__":
    main()
