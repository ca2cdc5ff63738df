"""Timings of sah_lighting_vrs and sah_vrsaa_resolve (include/sah_vrs.h) on cuda:0 against sah_lighting in the same run on the same planes: the
CSM + LPV + sky inputs of bench.py's 4k_deferred_gi workload at 3840 x 2160 and at 7680 x 4320 (the VRSAA frame of a 4K output).

    python tools/bench_lighting_vrs.py [--calls 50] [--rounds 7] [--extents 4k,8k]

Cases per extent: sah_lighting; sah_lighting_vrs with uniform 1 x 1, 2 x 2 and 4 x 4 images at depth_tolerance +inf; and with the image the
library's own two VRSAA passes make from that G-buffer (texels of 16 x 16, depth_tolerance 0.01).  For every image the share of pixels that
are shaded (s(q) = q) is computed with a torch restatement of the source map, and the variable-rate frame is compared with the gather of
the full-rate frame through that map — the parity of the tests at the benchmark's extent.  Then the resolve 7680 x 4320 -> 3840 x 2160 against
its byte floor at the copy rate of DESIGN.md §7, and the mode end to end — variable-rate lighting at 8K plus the resolve — against
sah_lighting at 4K plus sah_copy_scene.  The LPV gather copy of sah_lighting is kept between calls (lpv_generation 1), so no case pays a
rebuild.  Events around N back-to-back calls after a warm-up; the cases alternate round by round; median of the rounds with their range.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ACHIEVABLE_BYTES_PER_S = 6.3e12
EXTENTS = {"4k": (3840, 2160), "8k": (7680, 4320)}
TEXEL = (16, 16)
RATES = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 4), (4, 2), (4, 4)]


def source_map(depth, rates, texel, tol):
    """the source map of include/sah_vrs.h on device tensors: (sy, sx) int64, fp32 operators each rounded on its own"""
    import torch
    h, w = depth.shape
    yy, xx = torch.meshgrid(torch.arange(h, device=depth.device), torch.arange(w, device=depth.device), indexing="ij")
    code = rates[yy // texel[1], xx // texel[0]].long()
    lw, lh = torch.clamp((code >> 2) & 3, max=2), torch.clamp(code & 3, max=2)
    cw, ch = torch.ones_like(lw) << lw, torch.ones_like(lh) << lh
    ox, oy = xx & ~(cw - 1), yy & ~(ch - 1)
    surface = depth != 0
    ry, rx = torch.full_like(yy, -1), torch.full_like(xx, -1)
    for j in (3, 2, 1, 0):
        for k in (3, 2, 1, 0):
            py, px = oy + j, ox + k
            ok = (j < ch) & (k < cw) & (py < h) & (px < w)
            ok &= surface[py.clamp(max=h - 1), px.clamp(max=w - 1)]
            ry, rx = torch.where(ok, py, ry), torch.where(ok, px, rx)
    dr = depth[ry.clamp(min=0), rx.clamp(min=0)]
    share = surface & (ry >= 0) & ((depth - dr).abs() <= torch.tensor(tol, dtype=torch.float32, device=depth.device) * dr.abs())
    return torch.where(share, ry, yy), torch.where(share, rx, xx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--extents", default="4k,8k")
    args = ap.parse_args()
    import torch

    from androidrenderer_amd import _abi, frame, images, lib, scene

    torch.cuda.set_device(0)
    ctx = lib.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"calls": args.calls, "rounds": args.rounds, "unit": "ms per call, median of the rounds", "device": torch.cuda.get_device_name(0), "texel": TEXEL}
    RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT
    keep, cases, lits = [], {}, {}
    for tag in args.extents.split(","):
        w, h = EXTENTS[tag]
        fr = frame.LightingInputs(w, h, seed=2, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flavour="atrium", shadowmap_res=4096, synth_device="cuda")
        fr.lpv_generation = 1
        dev = fr.device_arrays()
        full, lit = (torch.zeros((h, w, 4), dtype=torch.int16, device="cuda") for _ in range(2))
        d_full, k1 = fr.describe(dev, full)
        d_vrs, k2 = fr.describe(dev, lit)
        sw, sh = scene.shading_rate_image_extent((w, h), TEXEL)
        # the library's own image: contrast of this G-buffer, then the rates
        contrast = torch.zeros((h, w, 2), dtype=torch.int16, device="cuda")
        library = torch.zeros((sh, sw), dtype=torch.uint8, device="cuda")
        cp = images.plane(contrast, _abi.FORMAT_R16G16_SFLOAT)
        ctx.vrsaa_measure_aliasing(images.plane(dev["color"], _abi.FORMAT_R8G8B8A8_SRGB), images.plane(dev["depth"], _abi.FORMAT_D32_SFLOAT), cp)
        ctx.vrsaa_shading_rate_image(cp, images.plane(library, _abi.FORMAT_R8_UINT), scene.shading_rate_params((w, h), (sw, sh), RATES))
        ctx.lighting(d_full)
        torch.cuda.synchronize()
        del contrast
        out[f"{tag}_sky_share"] = round(float((dev["depth"] == 0).float().mean()), 4)
        imgs = {"1x1": (torch.zeros_like(library), float("inf")), "2x2": (torch.full_like(library, 5), float("inf")),
                "4x4": (torch.full_like(library, 10), float("inf")), "library": (library, 0.01)}
        keep.append((fr, dev, full, lit, k1, k2, imgs))
        cases[f"lighting_{tag}"] = lambda d_full=d_full: ctx.lighting(d_full)
        for name, (img, tol) in imgs.items():
            plane = images.plane(img, _abi.FORMAT_R8_UINT)
            fn = (lambda d_vrs=d_vrs, plane=plane, tol=tol: ctx.lighting_vrs(d_vrs, plane, TEXEL, tol))
            cases[f"vrs_{name}_{tag}"] = fn
            fn()
            torch.cuda.synchronize()
            sy, sx = source_map(dev["depth"], img, TEXEL, tol)
            yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
            out[f"vrs_{name}_{tag}_shaded_share"] = round(float(((sy == yy) & (sx == xx)).float().mean()), 4)
            bad = int((lit != full[sy, sx]).any(-1).sum())
            out[f"vrs_{name}_{tag}_pixels_off_the_gather"] = bad
            assert bad == 0, f"{name} at {tag}: {bad} pixels are not the full-rate frame's at their source"
            del sy, sx, yy, xx
        lits[tag] = (d_full, d_vrs, full, lit, images.plane(library, _abi.FORMAT_R8_UINT))
    if "8k" in lits and "4k" in lits:
        resolved, copied = (torch.zeros((2160, 3840, 4), dtype=torch.int16, device="cuda") for _ in range(2))
        keep.append((resolved, copied))
        lit8_p, res_p = images.plane(lits["8k"][3], RGBA16F), images.plane(resolved, RGBA16F)
        full4_p, copy_p = images.plane(lits["4k"][2], RGBA16F), images.plane(copied, RGBA16F)
        d_vrs8, lib8, d_full4 = lits["8k"][1], lits["8k"][4], lits["4k"][0]
        cases["resolve_8k_to_4k"] = lambda: ctx.vrsaa_resolve(lit8_p, res_p)
        cases["copy_scene_4k"] = lambda: ctx.copy_scene(full4_p, copy_p)

        def vrsaa_mode():
            ctx.lighting_vrs(d_vrs8, lib8, TEXEL, 0.01)
            ctx.vrsaa_resolve(lit8_p, res_p)

        def plain_mode():
            ctx.lighting(d_full4)
            ctx.copy_scene(full4_p, copy_p)
        cases["vrs_library_8k_and_resolve"] = vrsaa_mode
        cases["lighting_4k_and_copy_scene"] = plain_mode
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
    for tag in lits:
        base = out[f"lighting_{tag}"]
        for name in ("1x1", "2x2", "4x4", "library"):
            out[f"vrs_{name}_over_lighting_{tag}"] = round(out[f"vrs_{name}_{tag}"] / base, 3)
        # t(f) = a + b f through the uniform 1 x 1 and 4 x 4 cases (f: the shaded share); the pass breaks even with sah_lighting at t(f) = base
        f1, f4, t1, t4 = out[f"vrs_1x1_{tag}_shaded_share"], out[f"vrs_4x4_{tag}_shaded_share"], out[f"vrs_1x1_{tag}"], out[f"vrs_4x4_{tag}"]
        b = (t1 - t4) / (f1 - f4)
        a = t4 - b * f4
        out[f"fixed_ms_{tag}"], out[f"ms_per_shaded_share_{tag}"] = round(a, 5), round(b, 5)
        out[f"break_even_shaded_share_{tag}"] = round((base - a) / b, 4)
    if "resolve_8k_to_4k" in out:
        nbytes = 8 * (7680 * 4320 + 3840 * 2160)
        out["resolve_floor_ms"] = round(nbytes / ACHIEVABLE_BYTES_PER_S * 1e3, 5)
        out["resolve_of_achievable"] = round(nbytes / (out["resolve_8k_to_4k"] * 1e-3) / ACHIEVABLE_BYTES_PER_S, 4)
        out["vrsaa_mode_over_plain_4k"] = round(out["vrs_library_8k_and_resolve"] / out["lighting_4k_and_copy_scene"], 3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
