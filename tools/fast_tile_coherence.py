"""How compact a wave of the fast Lighting kernel is in world space, by the shape of its pixel footprint — counted on the CPU, no GPU needed.

    python tools/fast_tile_coherence.py [workload]        (a Lighting workload of bench.py with a CSM sun and an LPV; default 4k_deferred_gi)

A plain fp32 numpy restatement of the kernel's geometry (lighting_fast.hpp: view-space position, world position, CSM cascade, PCF taps, LPV
cascade and footprint) over the workload's own frame: good for statistics, not for bits.  Per footprint of a wave at 4 pixels per thread
(256 x 1 is the strip of the linear map; fast_pixel_map.hpp keeps 64 x 4) it prints
  - the distinct 128-byte lines one PCF tap load touches over the wave's 64 lanes (mean over the four taps and the waves that run the PCF),
  - the same for one row load of the LPV footprint (48 bytes per lane; mean over the four rows),
  - the share of (wave, pixel slot) pairs whose vote runs the PCF (a lane with ndotl > 0) and the BRDF (a lit lane whose shadow is not 0),
    against the share of pixels that need them,
  - the share of waves that hold sky and surface pixels at once,
  - the share of (wave, pixel slot) pairs with a surface pixel that the wave's LPV texel box serves, under exactly the kernel's rule
    (csrc/lpv_box.hpp: a 4 x 4 x 4-texel box around the footprint base of one reference lane of slot 0, valid when every surface lane of slot 0 is
    served; a slot taps from the box when the box is valid and all its surface lanes are served), for both choices of the reference lane: the first
    surface lane, and the first surface lane at or behind the tile's centre lane (else the last before it), which the kernel keeps.  Every pixel
    that is not sky counts as a surface pixel here: the few the kernel defers are not modelled."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from androidrenderer_amd import _abi, frame  # noqa: E402

f32 = np.float32
# bench.py's Lighting workloads with a CSM sun and an LPV overlay: extent, G-buffer flavour, shadow map (restated: this tool imports the package only)
WORKLOADS = {"4k_deferred_gi": ((3840, 2160), "atrium", "noise"), "4k_deferred_gi_scene_shadow": ((3840, 2160), "atrium", "scene"),
             "4k_deferred_gi_random": ((3840, 2160), "random", "noise"), "1080p_deferred_gi": ((1920, 1080), "atrium", "noise"),
             "8k_deferred_gi": ((7680, 4320), "atrium", "noise")}
SHAPES = ((256, 1), (128, 2), (64, 4), (32, 8), (16, 16))
PPT = 4


def geometry(fr):
    """per pixel: surface, lit (PCF needed), brdf (BRDF needed), byte offsets of the four PCF taps and of the four LPV footprint rows, the
    footprint's base texel (x0, y0, z0) in the gather copy's padded coordinates and the volume's extents (w, h, d)"""
    W, H = fr.width, fr.height
    g = fr.view.gpu_data
    P, V = np.array(g.inverse_projection[:], f32), np.array(g.inverse_view[:], f32)
    res = np.array(g.render_resolution[:], f32)
    depth = fr.arrays["depth"].astype(f32)
    surface = (depth != 0) & np.isfinite(depth)
    with np.errstate(all="ignore"):
        tx = ((np.arange(W, dtype=f32) + f32(0.5)) + f32(0.5)) / res[0]
        ty = ((np.arange(H, dtype=f32) + f32(0.5)) + f32(0.5)) / res[1]
        colx, rowy = P[0] * (tx * f32(2) - f32(1)) + P[12], P[5] * (ty * f32(2) - f32(1)) + P[13]
        vw, vzn = P[11] * depth + P[15], P[10] * depth + P[14]
        vx, vy, vsz = colx[None, :] / vw, rowy[:, None] / vw, vzn / vw
        ws = [np.nan_to_num(V[i] * vx + V[4 + i] * vy + V[8 + i] * vsz + V[12 + i], posinf=0, neginf=0).astype(f32) for i in range(3)]
        n = fr.arrays["normals"].view(np.float16)[..., :3].astype(f32)
        n = n / np.sqrt((n * n).sum(-1, keepdims=True))
        n = np.nan_to_num(n)
        d = np.array(fr.sun.constants.direction_and_tan_size[:3], f32)
        L = -d / np.sqrt((d * d).sum())
        ndotl = np.clip(n @ L, 0, 1).astype(f32)
        lit = surface & (ndotl > 0)
        # CSM cascade and PCF taps
        splits = [f32(fr.sun.constants.data[c][0]) for c in range(4)]
        cascade = np.zeros((H, W), np.int32)
        for i in range(4):
            cascade = np.where(vsz < splits[i], i + 1, cascade)
        cc = np.minimum(cascade, 3)
        M = [np.array(fr.sun.constants.cascade_matrices[c][:], f32) for c in range(4)]  # column-major
        sp = [np.choose(cc, [M[c][r] * ws[0] + M[c][4 + r] * ws[1] + M[c][8 + r] * ws[2] + M[c][12 + r] for c in range(4)]) for r in range(3)]
        sm = fr.arrays["shadowmap"]
        sd, sh, sw = sm.shape
        px, py = sp[0] * f32(sw) - f32(0.5), sp[1] * f32(sh) - f32(0.5)
        fx0, fy0 = np.floor(px), np.floor(py)
        ci = lambda v, hi: np.clip(np.nan_to_num(v, posinf=hi, neginf=0), 0, hi).astype(np.int64)
        xa, xb, ya, yb = ci(fx0, sw - 1), ci(fx0 + 1, sw - 1), ci(fy0, sh - 1), ci(fy0 + 1, sh - 1)
        row_pitch, slice_pitch = sw * 2, sw * sh * 2
        taps = [cc * slice_pitch + y * row_pitch + x * 2 for y, x in ((ya, xa), (ya, xb), (yb, xa), (yb, xb))]
        bias = f32(0.0005) * np.sqrt(f32(1) - ndotl * ndotl) / ndotl
        ref = np.clip(sp[2] - bias, 0, 1)
        fx, fy = px - fx0, py - fy0
        wts = ((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)
        pcf = sum(w * (ref < sm[cc, y, x].astype(f32) / f32(65535)) for w, (y, x) in zip(wts, ((ya, xa), (ya, xb), (yb, xa), (yb, xb))))
        inside = ~((np.minimum(np.minimum(sp[0], sp[1]), sp[2]) < 0) | (np.maximum(np.maximum(sp[0], sp[1]), sp[2]) > 1))
        shadow = np.where(cascade > 3, 0, np.where(inside, pcf, 1))
        brdf = lit & (shadow != 0)
        # LPV cascade and the footprint's four (y, z) rows in the gather copy (k_lpv_pack: 24-byte texels inside a two-texel border)
        nc = len(fr.lpv.matrices)
        S = [np.array(fr.lpv.matrices[c].world_to_cascade[:], f32) for c in range(nc)]
        sel = np.zeros((H, W), np.int32)
        for i in range(nc - 1, -1, -1):
            c = [S[i][5 * k] * ws[k] + S[i][12 + k] for k in range(3)]
            ins = (np.minimum(np.minimum(c[0], c[1]), c[2]) > 0) & (np.maximum(np.maximum(c[0], c[1]), c[2]) < 1)
            sel = np.where(ins, i, sel)
        cp = [np.choose(sel, [S[c][5 * k] * (ws[k] + n[..., k]) + S[c][12 + k] for c in range(nc)]) for k in range(3)]
        cp[0] = (cp[0] + sel.astype(f32)) / f32(nc)
        ld, lh, lw = fr.arrays["lpv_r"].shape[:3]
        t0 = [ci(np.floor(cp[k] * f32(e) - f32(0.5)) + 2, e + 2) for k, e in enumerate((lw, lh, ld))]
        lrow = (lw + 4) * 24
        lslice = lrow * (lh + 4)
        base = t0[2] * lslice + t0[1] * lrow + t0[0] * 24
        rows = [base, base + lrow, base + lslice, base + lslice + lrow]
    return surface, lit, brdf, taps, rows, t0, (lw, lh, ld)


def per_wave(a, tw, th):
    """(H, W) -> (waves, PPT slots, 64 lanes) for waves of tw x th pixels at PPT pixels per thread"""
    H, W = a.shape
    return a.reshape(H // th, th, W // tw, tw // PPT, PPT).transpose(0, 2, 4, 1, 3).reshape(-1, PPT, 64)


def distinct(lines):
    """number of distinct values along the last axis"""
    s = np.sort(lines, axis=-1)
    return 1 + (s[..., 1:] != s[..., :-1]).sum(-1)


def box_served(base, extents, w_surf, tw, th, centre_rule):
    """share of (wave, slot) pairs with a surface pixel that tap from the wave's box (csrc/lpv_box.hpp)"""
    b = [per_wave(t, tw, th) for t in base]  # (waves, PPT, 64) per axis
    act0 = w_surf[:, 0, :]
    has0 = act0.any(-1)
    lane = np.arange(64)
    first = np.where(act0, lane, 64).min(-1)
    if centre_rule:
        centre = (th // 2) * (tw // PPT) + tw // (2 * PPT)
        behind = np.where(act0 & (lane >= centre), lane, 64).min(-1)
        last = np.where(act0, lane, -1).max(-1)
        ref = np.where(behind < 64, behind, last)
    else:
        ref = first
    ref = np.clip(ref, 0, 63)
    waves = np.arange(act0.shape[0])
    served = np.ones(w_surf.shape, bool)
    for axis, e in enumerate(extents):
        r = b[axis][waves, 0, ref]
        o = np.clip(r - 1, 0, e + 4 - 4)
        d = b[axis] - o[:, None, None]
        served &= (d >= 0) & (d <= 2)
    slot_ok = (served | ~w_surf).all(-1)  # every surface lane of the slot served
    valid = has0 & slot_ok[:, 0]
    pairs = w_surf.any(-1)
    return (pairs & slot_ok & valid[:, None]).sum() / max(1, pairs.sum())


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "4k_deferred_gi"
    (W, H), flavour, shadow = WORKLOADS[name]
    fr = frame.LightingInputs(W, H, seed=2, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flavour=flavour, shadowmap_res=4096, shadow=shadow)
    surface, lit, brdf, taps, rows, base, extents = geometry(fr)
    print(f"{name}: {W} x {H}, {flavour} G-buffer, shadow map '{shadow}'; pixels that need the PCF {100 * lit.mean():.1f} %, the BRDF {100 * brdf.mean():.1f} %, "
          f"sky {100 * (fr.arrays['depth'] == 0).mean():.1f} %")
    print("| wave footprint (px) | 128-B lines per PCF tap load | per LPV row load (48 B/lane) | wave slots that run the PCF | the BRDF | waves mixing sky and surface | "
          "LPV box serves: reference = first surface lane | = surface lane at the centre |")
    print("|---|---|---|---|---|---|---|---|")
    for tw, th in SHAPES:
        if W % tw or H % th:
            print(f"| {tw}x{th} | (the extent is not whole tiles) | | | | | | |")
            continue
        w_lit, w_brdf, w_surf = per_wave(lit, tw, th).any(-1), per_wave(brdf, tw, th).any(-1), per_wave(surface, tw, th)
        pcf_lines = np.mean([distinct(per_wave(t, tw, th) >> 7)[w_lit].mean() for t in taps])
        run_lpv = w_surf.any(-1)
        lpv_lines = np.mean([distinct(np.concatenate([per_wave(r, tw, th) >> 7, per_wave(r + 47, tw, th) >> 7], -1))[run_lpv].mean() for r in rows])
        any_surf, all_surf = w_surf.any((1, 2)), w_surf.all((1, 2))
        print(f"| {tw}x{th} | {pcf_lines:.1f} | {lpv_lines:.1f} | {100 * w_lit.mean():.1f} % | {100 * w_brdf.mean():.1f} % | {100 * (any_surf & ~all_surf).mean():.1f} % | "
              f"{100 * box_served(base, extents, w_surf, tw, th, False):.1f} % | {100 * box_served(base, extents, w_surf, tw, th, True):.1f} % |")


if __name__ == "__main__":
    main()
