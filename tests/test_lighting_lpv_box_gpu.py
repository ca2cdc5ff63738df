"""The fast Lighting kernel's per-wave LPV texel box on the GPU (androidrenderer_amd/csrc/lpv_box.hpp; tests/test_lpv_box_cpu.py checks the rule
itself on the host).  A wave whose first pixel slot fits one 4 x 4 x 4-texel box of the gather copy stages that box as fp32 in LDS, and every slot
whose surface lanes are all served taps from there; any other slot gathers as before.  Which path a wave took cannot be seen from outside, so the
frames here are constructed: a wall in front of a camera with a 0.2-degree field of view, whose depth is solved per pixel for the world-space x that
puts the pixel's footprint base on a chosen texel of cascade 0 (1-metre texels), and whose other two bases stay put over the frame.  A restatement of
the rule (_paths) then says, per wave and slot, which path the kernel must take, and every case asserts that it is the case it is named for before
it compares, per path (4, 2, 1 pixels per thread), the lit bytes with the general kernel and with the oracle: 0 differing bytes."""
import numpy as np
import pytest

from tests import lighting_cases as lc
from tests import util

pytestmark = pytest.mark.gpu

f32 = np.float32
PATHS = (("4 px per thread", False, 4), ("2 px per thread", False, 2), ("1 px per thread", False, 1), ("general", True, 0))
CAMERA = dict(position=(-7.0, 1.0, 0.0), fov=0.2, near=0.5)  # looks along +x; y = 1 and z = 0 are cell boundaries: the y / z fractions sit at 0.5
N_REF = 17  # the wall's footprint base on x (padded coordinates): world x = 2, nine metres in front of the camera
SHAPES = {"64x16": (64, 16, 0, 16), "128x8": (128, 8, 0, 8), "64x18-row1": (64, 18, 1, 18), "60x8-strips": (60, 8, 0, 8)}


# ---- construction ----------------------------------------------------------------------------------------------------------------------

def _frame(width, height, seed, sky=True):
    f = lc.MatrixFrame(width, height, flavour="random", seed=seed, shadowmap_res=128, sky=sky, camera=CAMERA, lpv=dict(cell=0.5), **lc.CSM_LPV)
    for k in ("color", "normals", "data", "emission", "depth", "lpv_r", "lpv_g", "lpv_b"):
        f.arrays[k] = f.arrays[k].copy()
    f.arrays["data"][..., 1] = np.maximum(f.arrays["data"][..., 1], 1)  # roughness bytes >= 1: what a frame defers is what the case plants
    n = f.arrays["normals"].view(np.uint16)
    n[..., 0], n[..., 1], n[..., 2] = 0xBC00, 0, 0  # the normal (-1, 0, 0): the gather point is the surface point moved one metre towards the camera
    return f


def _world_x_of_base(f, n):
    """world x of a surface point whose footprint base on x is n (padded coordinates) with the fraction at 0.5, inside cascade 0"""
    S = np.array(f.lpv.matrices[0].world_to_cascade[:], np.float64)
    return ((n - 1) / 32.0 - S[12]) / S[0] + 1.0


def _set_wall(f, world_x):
    """depth of every pixel so that its world-space x is world_x[y, x] (the view-space position is the pixel's ray / vw: solved for vw in fp64)"""
    g = f.view.gpu_data
    P, V, res = np.array(g.inverse_projection[:], np.float64), np.array(g.inverse_view[:], np.float64), np.array(g.render_resolution[:], np.float64)
    assert P[10] == 0.0
    tx = ((np.arange(f.width) + 0.5) + 0.5) / res[0]
    ty = ((np.arange(f.height) + 0.5) + 0.5) / res[1]
    colx, rowy = P[0] * (tx * 2 - 1) + P[12], P[5] * (ty * 2 - 1) + P[13]
    ray_x = V[0] * colx[None, :] + V[4] * rowy[:, None] + V[8] * P[14]
    vw = ray_x / (np.asarray(world_x, np.float64) - V[12])
    depth = ((vw - P[15]) / P[11]).astype(f32)
    assert np.isfinite(depth).all() and (depth > 0).all()
    f.arrays["depth"][...] = depth


def _wall_of_bases(f, bases_x):
    _set_wall(f, _world_x_of_base(f, np.asarray(bases_x, np.float64)))


def _refit_lpv_around(f, shift):
    """the LPV cascades fitted around a camera `shift` metres away: every pixel then lies far outside every cascade"""
    pos = tuple(p + s for p, s in zip(f.camera["position"], shift))
    f.lpv.update_cascade_transforms(lc.make_view(f.width, f.height, **dict(f.camera, position=pos)), f.sun)


# ---- the kernel's geometry and rule, restated (fp32 numpy; the constructed positions are far from every rounding boundary) -----------------

def _bases(f):
    """per pixel: the footprint base (x0, y0, z0) in the gather copy's padded coordinates, and the padded extents"""
    g = f.view.gpu_data
    P, V, res = np.array(g.inverse_projection[:], f32), np.array(g.inverse_view[:], f32), np.array(g.render_resolution[:], f32)
    depth = f.arrays["depth"].astype(f32)
    with np.errstate(all="ignore"):
        tx = ((np.arange(f.width, dtype=f32) + f32(0.5)) + f32(0.5)) / res[0]
        ty = ((np.arange(f.height, dtype=f32) + f32(0.5)) + f32(0.5)) / res[1]
        colx, rowy = P[0] * (tx * f32(2) - f32(1)) + P[12], P[5] * (ty * f32(2) - f32(1)) + P[13]
        vw, vzn = P[11] * depth + P[15], P[10] * depth + P[14]
        vx, vy, vsz = colx[None, :] / vw, rowy[:, None] / vw, vzn / vw
        ws = [np.nan_to_num(V[i] * vx + V[4 + i] * vy + V[8 + i] * vsz + V[12 + i], posinf=0, neginf=0).astype(f32) for i in range(3)]
        n = f.arrays["normals"].view(np.float16)[..., :3].astype(f32)
        n = np.nan_to_num(n / np.sqrt((n * n).sum(-1, keepdims=True)))
        nc = len(f.lpv.matrices)
        S = [np.array(f.lpv.matrices[c].world_to_cascade[:], f32) for c in range(nc)]
        sel = np.zeros(depth.shape, np.int32)
        for i in range(nc - 1, -1, -1):
            c = [S[i][5 * k] * ws[k] + S[i][12 + k] for k in range(3)]
            ins = (np.minimum(np.minimum(c[0], c[1]), c[2]) > 0) & (np.maximum(np.maximum(c[0], c[1]), c[2]) < 1)
            sel = np.where(ins, i, sel)
        cp = [np.choose(sel, [S[c][5 * k] * (ws[k] + n[..., k]) + S[c][12 + k] for c in range(nc)]) for k in range(3)]
        cp[0] = (cp[0] + sel.astype(f32)) / f32(nc)
        ld, lh, lw = f.arrays["lpv_r"].shape[:3]
        ext = (lw, lh, ld)
        base = [np.clip(np.nan_to_num(np.floor(cp[k] * f32(e) - f32(0.5)), posinf=1e9, neginf=-1e9), -2, e).astype(np.int64) + 2 for k, e in enumerate(ext)]
    return base, tuple(e + 4 for e in ext), sel


def _active(f):
    """the lanes whose surface terms are used: surface pixels the fast kernel does not defer for its inputs"""
    depth, nrm = f.arrays["depth"], f.arrays["normals"].view(np.float16)[..., :3].astype(f32)
    dn = (nrm * nrm).sum(-1)
    return np.isfinite(depth) & (depth != 0) & (dn > 0) & np.isfinite(dn) & (f.arrays["data"][..., 1] != 0)


def _paths(f, r0, r1, ppt, active=None):
    """[(path, has a surface lane)] per (wave, slot) of a launch over rows [r0, r1): fast_pixel_map.hpp and lpv_box.hpp restated"""
    base, padded, _ = _bases(f)
    act = _active(f) if active is None else active
    width, rows = f.width, r1 - r0
    gpr = width // ppt
    R = ppt if (width % 64 == 0 and rows >= ppt) else 0
    lpr = 64 // ppt
    centre = (ppt // 2) * (64 // ppt) + 32 // ppt

    def pixel(gid):
        ry = gid // gpr
        band = ry & ~(R - 1) if R else 0
        if R == 0 or band + R > rows:
            return (gid - ry * gpr) * ppt, ry
        r = gid - band * gpr
        tile, lane = r >> 6, r & 63
        return (tile * lpr + (lane & (lpr - 1))) * ppt, band + lane // lpr

    out = []
    for w0 in range(0, gpr * rows, 64):
        lanes = [pixel(g) for g in range(w0, min(w0 + 64, gpr * rows))]
        valid, o = False, (0, 0, 0)
        for slot in range(ppt):
            a = [bool(act[r0 + y, x + slot]) for x, y in lanes]
            b = [tuple(int(base[k][r0 + y, x + slot]) for k in range(3)) for x, y in lanes]
            live = [l for l in range(len(lanes)) if a[l]]
            if slot == 0 and live:
                behind = [l for l in live if l >= centre]
                ref = behind[0] if behind else live[-1]
                o = tuple(min(max(b[ref][k] - 1, 0), padded[k] - 4) for k in range(3))
            served = all(0 <= b[l][k] - o[k] <= 2 for l in live for k in range(3))
            if slot == 0:
                valid = len(lanes) == 64 and bool(live) and served
            out.append(("box" if valid and served else "gather", bool(live)))
    return out


def _shares(paths):
    live = [p for p, has in paths if has]
    return sum(p == "box" for p in live), len(live)


# ---- running -----------------------------------------------------------------------------------------------------------------------------

def _run(f, ctx, name, r0=0, r1=None, expect=None, active=None, ref=None):
    """every path over rows [r0, r1): the same bytes as the general kernel and as the oracle.  `expect`: {ppt: "box" | "gather" | "both"}, what the
    restated rule must say of the slots that hold a surface lane — the case is the one it is named for"""
    r1 = f.height if r1 is None else r1
    ref = f.run_oracle() if ref is None else ref
    dev = f.device_arrays()
    whole = (r0, r1) == (0, f.height)
    f.row_begin, f.row_end = (0, 0) if whole else (r0, r1)
    outs = {}
    try:
        for path, general, forced in PATHS:
            ctx.debug_set(force_general=general, force_ppt=forced)
            got = f.run_hip(ctx, dev)
            rep = ctx.lighting_dispatch()
            if general:
                assert rep["family"] == "general", rep
            else:
                assert rep["family"] == "fast" and rep["ppt"] == lc.expected_ppt(f.width, r1 - r0, True, forced), f"{name} [{path}]: {rep}"
                box, live = _shares(_paths(f, r0, r1, forced, active))
                print(f"{name} [{path}]: {box} of {live} slots with a surface lane tap from the box, {ctx.deferred_pixels()} deferred pixels")
                want = (expect or {}).get(forced)
                if want == "box":
                    assert live > 0 and box == live, f"{name} [{path}]: constructed for the box, {box} of {live} slots"
                elif want == "gather":
                    assert box == 0, f"{name} [{path}]: constructed for the gather, {box} of {live} slots tap from the box"
                elif want == "both":
                    assert 0 < box < live, f"{name} [{path}]: constructed for both paths, {box} of {live} slots tap from the box"
            nd = int((got[r0:r1] != ref[r0:r1]).sum())
            print(f"{name} [{path}]: {nd} of {got[r0:r1].size} values differ from the oracle")
            assert nd == 0, f"{name} [{path}]: {nd} values differ from the oracle; " + util.report_ulp(name, util.f16_ulp_diff(got[r0:r1], ref[r0:r1]))
            if not whole:
                assert not got[:r0].any() and not got[r1:].any(), f"{name} [{path}]: a row outside [{r0}, {r1}) was written"
            outs[path] = got
    finally:
        ctx.debug_set(force_general=False, force_ppt=0)
        f.row_begin = f.row_end = 0
    for path in outs:
        assert np.array_equal(outs[path], outs["general"]), f"{name}: the {path} path and the general kernel disagree"
    return outs


ALL_BOX = {4: "box", 2: "box", 1: "box"}
ALL_GATHER = {4: "gather", 2: "gather", 1: "gather"}
BOTH = {4: "both", 2: "both", 1: "both"}


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_wall_inside_one_cell(hip_ctx, shape):
    """every pixel on one footprint base: whole waves are served; the strip launch's last wave is not whole and gathers"""
    width, height, r0, r1 = SHAPES[shape]
    f = _frame(width, height, 5100 + width + height)
    _wall_of_bases(f, np.full((height, width), N_REF))
    base, _, sel = _bases(f)
    assert all(len(np.unique(b)) == 1 for b in base) and base[0][0, 0] == N_REF and not sel.any()
    # (64 x 18 from row 1: the seventeenth row is behind the last full band at 4 and 2 pixels per thread, a quarter / half of a wave, which gathers)
    _run(f, hip_ctx, shape, r0, r1, expect=BOTH if width % 64 else ({4: "both", 2: "both", 1: "box"} if (r1 - r0) % 4 else ALL_BOX))


@pytest.mark.parametrize("sky", [True, False], ids=["sky", "no-sky"])
@pytest.mark.parametrize("shape", ["64x16", "128x8"])
def test_neighbouring_bases_are_served(hip_ctx, shape, sky):
    """bases r - 1, r and r + 1 around the reference pixel (column 32 of a tile at every pixel count), in every slot"""
    width, height, r0, r1 = SHAPES[shape]
    f = _frame(width, height, 5200 + width, sky=sky)
    cols = np.array([N_REF + (-1, 0, 1, 0, 1, -1, 0)[x % 7] for x in range(width)])
    cols[32::64] = N_REF
    _wall_of_bases(f, np.broadcast_to(cols, (height, width)))
    assert set(np.unique(_bases(f)[0][0]) - N_REF) == {-1, 0, 1}
    _run(f, hip_ctx, f"{shape} r-1..r+1", r0, r1, expect=ALL_BOX)


@pytest.mark.parametrize("shape", ["64x16", "128x8"])
def test_bases_two_texels_away_fall_back(hip_ctx, shape):
    """r + 2 and r - 2: in a later slot (that slot gathers, the wave's other slots tap from the box) and in the first slot (the wave has no box)"""
    width, height, r0, r1 = SHAPES[shape]
    f = _frame(width, height, 5300 + width)
    want = np.full((height, width), N_REF)
    want[0:2, 5], want[0:2, 50] = N_REF + 2, N_REF - 2  # columns 5 and 50: slot 1 / 2 at 4 pixels per thread, slot 1 / 0 at 2
    want[4:6, 8] = N_REF + 2                            # column 8: the first slot at every pixel count
    want[6:8, 40] = N_REF - 2
    want[:, 33] = N_REF + 1
    _wall_of_bases(f, want)
    assert np.array_equal(_bases(f)[0][0], want)
    _run(f, hip_ctx, f"{shape} r+-2", r0, r1, expect=BOTH)


@pytest.mark.parametrize("shape", ["64x16", "128x8", "64x18-row1"])
def test_depth_step_and_cascade_boundary(hip_ctx, shape):
    """a depth step of six texels through the middle of every wave's tile, and rows whose right half lies in cascade 1"""
    width, height, r0, r1 = SHAPES[shape]
    f = _frame(width, height, 5400 + width + height)
    wx = np.full((height, width), _world_x_of_base(f, N_REF))
    wx[:, 32::64] = _world_x_of_base(f, N_REF + 6)
    for x in range(33, width):
        if x % 64 >= 32:
            wx[:, x] = wx[:, 32]
    wx[height // 2:, :] = _world_x_of_base(f, N_REF)
    S = np.array(f.lpv.matrices[0].world_to_cascade[:], np.float64)
    wx[height // 2:, width // 2:] = (1.0 - S[12]) / S[0] + 4.5  # 4.5 m behind the far face of cascade 0
    _set_wall(f, wx)
    base, _, sel = _bases(f)
    assert set(np.unique(base[0][: height // 2])) == {N_REF, N_REF + 6} and set(np.unique(sel[height // 2:])) == {0, 1}
    _run(f, hip_ctx, f"{shape} step", r0, r1, expect={4: "both", 2: "both"} if shape == "128x8" else {4: "gather", 2: "gather"})


@pytest.mark.parametrize("side", [300.0, -300.0], ids=["below", "above"])
def test_far_outside_every_cascade(hip_ctx, side):
    """every base clamped to 0 (the cascades lie 300 m further along every axis) or to size + 2 (300 m back): the origin clamp at either end, taps in
    the zero border"""
    f = _frame(64, 16, 5500)
    _wall_of_bases(f, np.full((16, 64), N_REF))
    _refit_lpv_around(f, (side, side, side))
    base, padded, _ = _bases(f)
    for k in range(3):
        assert set(np.unique(base[k])) == ({0} if side > 0 else {padded[k] - 2}), (k, np.unique(base[k]))
    _run(f, hip_ctx, f"far {side:+.0f}", expect=ALL_BOX)


def test_reference_lane_deferred_or_sky(hip_ctx):
    """column 32 — the reference pixel of every tile — is a NaN depth, a zero normal, a roughness byte 0 and sky in turn: the reference moves on to
    the next surface lane; and first slots that are all sky with surface in the others"""
    f = _frame(64, 16, 5600)
    want = np.full((16, 64), N_REF)
    want[:, 36:40] = N_REF + 1
    _wall_of_bases(f, want)
    f.arrays["depth"][0:4, 32] = np.float32("nan")
    f.arrays["normals"][4:8, 32, :3] = 0
    f.arrays["data"][8:12, 32, 1] = 0
    f.arrays["depth"][12:16, 32] = 0.0
    _run(f, hip_ctx, "reference deferred", expect=ALL_BOX)
    g = _frame(64, 16, 5601)
    _wall_of_bases(g, want)
    g.arrays["depth"][0:4, 0::4] = 0.0   # the first slot at 4 pixels per thread
    g.arrays["depth"][4:8, 0::2] = 0.0   # at 4 and at 2
    g.arrays["depth"][8:10, :] = 0.0     # whole rows: at 1, whole waves
    _run(g, hip_ctx, "first slot all sky", expect={4: "both", 2: "both", 1: "box"})


def test_nonfinite_volume_defers_every_pixel(hip_ctx):
    f = _frame(64, 16, 5700)
    _wall_of_bases(f, np.full((16, 64), N_REF))
    f.arrays["lpv_g"][3, 4, 5, 1] = np.float16("inf")
    _run(f, hip_ctx, "non-finite texel", expect=ALL_GATHER, active=np.zeros((16, 64), bool))
    assert hip_ctx.deferred_pixels() == 0  # (the last path run was the general kernel)
    hip_ctx.debug_set(force_ppt=4)
    try:
        f.run_hip(hip_ctx)
        assert hip_ctx.deferred_pixels() == 64 * 16
    finally:
        hip_ctx.debug_set()


def test_random_frame_mixes_both_paths(hip_ctx):
    """the atrium through a 1-degree field of view under the default cascades: whatever mix of served and unserved slots the frame gives (whole launches
    of either kind and launches of both)"""
    for width, height, r0, r1 in (SHAPES["128x8"], SHAPES["64x18-row1"], SHAPES["60x8-strips"]):
        f = lc.MatrixFrame(width, height, flavour="atrium", seed=5800 + width, shadowmap_res=128, camera=dict(fov=1.0, near=1.0), **lc.CSM_LPV)
        _run(f, hip_ctx, f"atrium {width}x{height}", r0, r1)


def test_kept_gather_copy():
    """the same frame twice with the same lpv_generation: the second call stages its boxes from the copy the first one built"""
    import torch
    from androidrenderer_amd import lib
    ctx = lib.Context(device=0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        f = _frame(64, 16, 5900)
        cols = np.array([N_REF + (0, 1, -1)[x % 3] for x in range(64)])
        cols[32] = N_REF
        _wall_of_bases(f, np.broadcast_to(cols, (16, 64)))
        assert _shares(_paths(f, 0, 16, 4)) == (16, 16)
        f.lpv_generation = 31
        ref = f.run_oracle()
        dev = f.device_arrays()
        ctx.debug_set(force_ppt=4)
        packs = ctx.copy_rebuilds()[0]
        outs = []
        for call in (0, 1):
            got = f.run_hip(ctx, dev)
            rep = ctx.lighting_dispatch()
            assert rep["family"] == "fast" and rep["ppt"] == 4 and rep["repack"] == (1 if call == 0 else 0), (call, rep)
            assert np.array_equal(got, ref), f"call {call}: {int((got != ref).sum())} values differ from the oracle"
            outs.append(got)
        assert ctx.copy_rebuilds()[0] == packs + 1, "the LPV gather copy was rebuilt although lpv_generation stood"
        ctx.debug_set(force_general=True)
        assert np.array_equal(f.run_hip(ctx, dev), outs[0]), "the fast path and the general kernel disagree"
    finally:
        ctx.debug_set()
        torch.cuda.synchronize()
        ctx.close()
