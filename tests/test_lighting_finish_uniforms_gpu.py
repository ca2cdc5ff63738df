"""The FINISH bodies of the fast Lighting kernel read the uniforms of their finish — the general restatement of the pixels a wave has listed —
late: from the kernarg segment, behind the listing vote, not from the arguments the prologue loaded (csrc/lighting.hip: FinishArgs).  A wrong
offset, a stale block or a uniform that is never fetched shows as other bytes in a finished pixel.  So: small frames in which the finish needs
every uniform it fetches, for the four bodies that had reserved scratch before (sun off / CSM / traced sun under an LPV, at the pixels per
thread named), each compared with the two-launch twin of the same body and with the general kernel at 0 differing bytes.

Frames: the atrium (which by itself lists nothing) at 64 x 8, and at 128 x 8 with every plane at a non-minimal pitch.  At P pixels per thread a
wave is a tile of 64 pixels x P rows, lanes row-major, 64 / P lanes per tile row (csrc/fast_pixel_map.hpp); wave 0 is listed whole, wave 1 lists
nothing, and where there are more the last wave lists two single pixels, on lane 0 (first pixel slot) and on lane 63 (last slot).  In wave 0:
  lane 0, first slot   depth +inf                       lane 0, last slot    NaN AO texel
  lane 63, first slot  zero normal                      every other pixel    roughness byte 0 (under the LPV: listed)
  lanes 1-4, first slot: facing the sun at view distances 1, 4, 10 and 60 m — one lit pixel in each shadow cascade (the CPU test below restates the
  cascade choice); lane 5, first slot: at 100 m, outside every LPV cascade.  Wave 1 holds the frame's sky pixels (the sky bound: they are the sky
  workgroups', not listed).
A second frame — another camera, sun and LPV layout (two cascades of 0.5 m cells) — runs on the same context after the first: a uniform kept from
the first call would show."""
import numpy as np
import pytest

from androidrenderer_amd import _abi
from tests import lighting_cases as lc

# body name -> (sun mode, pixels per thread); all with an LPV and a sky bound: k_lighting_fast<sun, 1, ppt, true, true>
BODIES = {"off_lpv_2": (_abi.SHADOW_MODE_OFF, 2), "csm_lpv_4": (_abi.SHADOW_MODE_CSM, 4), "csm_lpv_2": (_abi.SHADOW_MODE_CSM, 2),
          "rt_lpv_4": (_abi.SHADOW_MODE_RT, 4)}
PLANES = ("color", "normals", "data", "emission", "depth", "ao", "shadow_mask", "lit")
# (multiples of 16: 16-byte accesses, and with them 4 and 2 pixels per thread, stay available)
EXTENTS = {"64x8": (64, 8, {}), "128x8_pitched": (128, 8, {k: dict(row_pad=16 * (3 + i), offset=32) for i, k in enumerate(PLANES)})}
CAMERAS = {"first": dict(edit="plus_zero"), "second": dict(position=(3.5, 4.25, -2.0), yaw=37.0, pitch=-20.0, fov=60.0, near=0.1, edit="plus_zero")}
DISTANCES = (1.0, 4.0, 10.0, 60.0)  # metres in front of the camera: one in each shadow cascade (splits at 1.9, 5.6, 21.9, 128 m for near 0.05)
FAR = 100.0
_frames = {}


def pixel_of(width, ppt, wave, lane, slot):
    """(x, y) of pixel `slot` of `lane` of `wave` in a tiled launch over all rows (csrc/fast_pixel_map.hpp, tile_rows = ppt)"""
    band, tile = divmod(wave, width // 64)
    lpr = 64 // ppt
    return tile * 64 + (lane % lpr) * ppt + slot, band * ppt + lane // lpr


def depth_at(f, metres):
    """the depth value whose view-space z is -metres: z = (p10 D + p14) / (p11 D + p15)"""
    p = f.view.gpu_data.inverse_projection
    return np.float32((p[14] + metres * p[15]) / (-metres * p[11] - p[10]))


def build(body, extent, which):
    """the frame, where its strays are ({(x, y): kind}), its lit-per-cascade pixels and its far pixel — made once, never changed"""
    key = (body, extent, which)
    if key in _frames:
        return _frames[key]
    sun_mode, ppt = BODIES[body]
    w, h, pitch = EXTENTS[extent]
    kw = dict(sun_dir=(-0.4, -1.0, 0.3), sun_color=(60000.0, 70000.0, 50000.0), lpv=dict(num_cascades=2, cell=0.5)) if which == "second" else {}
    f = lc.MatrixFrame(w, h, camera=CAMERAS[which], seed=32 if which == "first" else 33, flavour="atrium", sky=True, sun_mode=sun_mode, gi=_abi.GI_LPV, **kw)
    a = {k: f.arrays[k] for k in ("depth", "normals", "data", "ao")}
    waves = (w // 64) * (h // ppt)
    strays = {}

    def place(wave, lane, slot, kind, metres=2.5):
        x, y = pixel_of(w, ppt, wave, lane, slot)
        assert (x, y) not in strays
        strays[(x, y)] = kind
        if a["depth"][y, x] == 0 or metres != 2.5:  # a surface pixel, at its own depth unless the set-up names one
            a["depth"][y, x] = depth_at(f, metres)
        if not np.any(a["normals"][y, x, :3]):
            a["normals"][y, x, :3] = (0.0, 1.0, 0.0)
        a["data"][y, x, 1] = max(int(a["data"][y, x, 1]), 1)
        if kind == "depth":
            a["depth"][y, x] = np.inf if wave == 0 else np.nan
        elif kind == "normal":
            a["normals"][y, x, :3] = 0.0
        elif kind == "ao":
            a["ao"][y, x] = np.nan
        else:
            a["data"][y, x, 1] = 0
        return x, y

    sun_l = -np.array(f.sun.constants.direction_and_tan_size[0:3], np.float64)
    lit, special = [], {(0, 0): "depth", (0, ppt - 1): "ao", (63, 0): "normal"}
    for lane in range(64):
        for slot in range(ppt):
            metres = DISTANCES[lane - 1] if 1 <= lane <= 4 and slot == 0 else (FAR if lane == 5 and slot == 0 else 2.5)
            x, y = place(0, lane, slot, special.get((lane, slot), "rough"), metres)
            if 1 <= lane <= 4 and slot == 0:
                a["normals"][y, x, :3] = sun_l / np.linalg.norm(sun_l)
                lit.append((x, y))
            if lane == 5 and slot == 0:
                far = (x, y)
    if waves > 2:
        place(waves - 1, 0, 0, "normal")
        place(waves - 1, 63, ppt - 1, "depth")
    # what is left of wave 1 lists nothing: no roughness byte 0 on a surface pixel, and it holds sky
    xs, ys = zip(*(pixel_of(w, ppt, 1, lane, slot) for lane in range(64) for slot in range(ppt)))
    tile = (np.array(ys), np.array(xs))
    a["data"][..., 1][tile] = np.maximum(a["data"][..., 1][tile], 1)
    x, y = pixel_of(w, ppt, 1, 7, 0)
    a["depth"][y, x] = 0.0
    f.pitch = dict(pitch)
    _frames[key] = dict(frame=f, strays=strays, lit=lit, far=far, ppt=ppt, dev=None, want=None, wave1=tile)
    return _frames[key]


def _positions(f, x, y):
    """view-space and world-space position of a pixel as the sun and LPV passes derive it (texcoord (x + 1) / W), in double precision"""
    g = f.view.gpu_data
    P = np.array(list(g.inverse_projection), np.float64).reshape(4, 4).T
    V = np.array(list(g.inverse_view), np.float64).reshape(4, 4).T
    ndc = np.array([(x + 1.0) / g.render_resolution[0] * 2.0 - 1.0, (y + 1.0) / g.render_resolution[1] * 2.0 - 1.0, float(f.arrays["depth"][y, x]), 1.0])
    vs = P @ ndc
    vs = vs / vs[3]
    return vs, V @ vs


CASES = [(b, e) for b in BODIES for e in EXTENTS]


@pytest.mark.parametrize("body,extent", CASES)
@pytest.mark.parametrize("which", ["first", "second"])
def test_frames_hold_the_set_ups(body, extent, which):
    """CPU: the strays sit where the docstring says, a lit stray lies in each shadow cascade, one stray outside every LPV cascade, sky in wave 1"""
    c = build(body, extent, which)
    f, ppt = c["frame"], c["ppt"]
    w, h, _ = EXTENTS[extent]
    depth, rough = f.arrays["depth"], f.arrays["data"][..., 1]
    assert len(c["strays"]) == 64 * ppt + (2 if (w // 64) * (h // ppt) > 2 else 0)
    kinds = {k: sum(1 for v in c["strays"].values() if v == k) for k in ("depth", "normal", "ao", "rough")}
    assert kinds["depth"] >= 1 and kinds["normal"] >= 1 and kinds["ao"] == 1 and kinds["rough"] >= 64 * ppt - 3
    for (x, y), kind in c["strays"].items():
        assert depth[y, x] != 0  # a surface pixel: the fast kernel lists it, the sky workgroups leave it alone
        assert {"depth": not np.isfinite(depth[y, x]), "normal": not np.any(f.arrays["normals"][y, x, :3]), "ao": np.isnan(f.arrays["ao"][y, x]),
                "rough": rough[y, x] == 0}[kind]
    # every surface pixel that is not a stray lists nothing by its inputs: finite depth, a normal, roughness byte != 0, finite AO
    rest = np.ones(depth.shape, bool)
    for (x, y) in c["strays"]:
        rest[y, x] = False
    rest &= depth != 0
    assert np.isfinite(depth[rest]).all() and (rough[rest] != 0).all() and np.isfinite(f.arrays["ao"][rest]).all()
    assert np.any(f.arrays["normals"][..., :3].astype(np.float32) != 0, axis=-1)[rest].all()
    assert (depth[c["wave1"]] == 0).any() and f.has_sky and not any((x, y) in c["strays"] for y, x in zip(*c["wave1"]))
    sun_l = -np.array(f.sun.constants.direction_and_tan_size[0:3], np.float64)
    if f.sun_mode == _abi.SHADOW_MODE_CSM:
        splits = [f.sun.constants.data[i][0] for i in range(4)]
        cascades = []
        for (x, y) in c["lit"]:
            vs, _ = _positions(f, x, y)
            cascades.append(sum(1 for s in splits if vs[2] < s))  # (sample_csm: the last split the depth lies behind, plus one)
            assert float(f.arrays["normals"][y, x, :3].astype(np.float64) @ sun_l) > 0.5 and c["strays"][(x, y)] == "rough"
        assert cascades == [0, 1, 2, 3], cascades
    n = getattr(f, "lpv_num_cascades", 4)
    _, ws = _positions(f, *c["far"])
    inside = []
    for ci in range(n):
        t = np.array(list(f.lpv.matrices[ci].world_to_cascade), np.float64).reshape(4, 4).T @ ws
        inside.append(bool(((t[:3] >= 0) & (t[:3] <= 1)).all()))
    assert not any(inside), inside
    _, ws = _positions(f, *c["lit"][1])
    t = np.array(list(f.lpv.matrices[n - 1].world_to_cascade), np.float64).reshape(4, 4).T @ ws
    assert ((t[:3] >= 0) & (t[:3] <= 1)).all()  # ... and one inside the widest


def _run(ctx, c, **debug):
    f = c["frame"]
    if c["dev"] is None:
        c["dev"] = f.device_arrays()
    ctx.debug_set(**debug)
    got = f.run_hip(ctx, c["dev"])  # (asserts the padding of the pitched planes)
    return got, ctx.lighting_dispatch(), ctx.deferred_pixels() if not debug.get("force_general") else 0


def _want(ctx, c):
    if c["want"] is None:
        c["want"], rep, _ = _run(ctx, c, force_general=True)
        assert rep["family"] == "general"
    return c["want"]


@pytest.mark.gpu
@pytest.mark.parametrize("body,extent", CASES)
def test_finish_reads_every_uniform_it_needs(hip_ctx, body, extent):
    first, second = build(body, extent, "first"), build(body, extent, "second")
    ppt = first["ppt"]
    try:
        wants = [_want(hip_ctx, c) for c in (first, second)]
        for c, want in zip((first, second), wants):  # (the second frame on the same context, behind the first: other sun, LPV layout and camera)
            by_launch, rep_l, n_l = _run(hip_ctx, c, force_ppt=ppt, strays="launch")
            inline, rep_i, n_i = _run(hip_ctx, c, force_ppt=ppt, strays="inline")
            print(f"{body} {extent}: {n_i} listed of {len(c['strays'])} placed; launch {rep_l['strays']}, inline {rep_i['strays']}")
            for rep in (rep_l, rep_i):
                assert rep["family"] == "fast" and rep["ppt"] == ppt, rep
            assert rep_l["strays"] == "launch" and rep_i["strays"] == "inline"
            assert n_i == n_l == len(c["strays"])  # (what was placed and nothing else: wave 1 lists nothing)
            assert np.array_equal(by_launch, want), f"{int((by_launch != want).any(-1).sum())} pixels of the two-launch twin differ from the general kernel's"
            assert np.array_equal(inline, want), f"{int((inline != want).any(-1).sum())} pixels differ from the general kernel's"
            assert np.array_equal(inline, by_launch)
    finally:
        hip_ctx.debug_set()
