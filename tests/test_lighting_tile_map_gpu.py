"""The fast Lighting kernel's thread -> pixel map on the GPU (androidrenderer_amd/csrc/fast_pixel_map.hpp; tests/test_fast_pixel_map_cpu.py checks
the map itself on the host).  Where a launch gathers — a CSM sun, an LPV overlay — and its width is whole 64-pixel tiles, a wave shades a tile of
64 pixels x ppt rows (64 x 4 at 4 pixels per thread, 64 x 2 at 2) instead of a strip of one row.  Three places turn a thread index into a
pixel: the surface workgroups, the sky workgroups' walk and the fix-up kernel, which turns a listed code back into its pixel.  A map that disagrees between them misplaces pixels: a
deferred pixel fixed up somewhere else, a sky pixel the walk never visits.  So every frame here plants pixels the fast kernel must defer
(roughness byte 0 under LPV GI, a NaN depth, a zero normal) and sky pixels (depth 0) at tile corners, either side of tile edges, in the rows behind
the last full band and on the last pixel, and asserts per path: bit-equal to the general kernel, within MAX_ULP of the oracle, and exactly the
planted pixels handed to the fix-up kernel."""
import numpy as np
import pytest

from tests import lighting_cases as lc
from tests import util

pytestmark = pytest.mark.gpu

MAX_ULP = util.MAX_ULP

PATHS = (("auto", False, 0), ("4 px per thread", False, 4), ("2 px per thread", False, 2), ("1 px per thread", False, 1), ("general", True, 0))

# corners of 32 x 8 tiles (a shape measured beside the kept one; positions inside the kept tiles), then the corners of the 64 x 4 tiles of 4 pixels
# per thread and the 64 x 2 tiles of 2, both sides of the edges between tiles, and the same in a second column of tiles (widths >= 128);
# (x, row of the launch)
CORNERS = ((0, 0), (31, 7), (32, 0), (63, 15), (31, 0), (32, 7), (0, 7), (0, 8), (31, 8), (32, 8), (63, 0), (63, 7), (30, 3), (33, 4), (4, 1), (35, 2),
           (63, 3), (0, 4), (0, 3), (63, 4), (63, 1), (0, 2), (60, 5), (3, 6), (64, 0), (127, 3), (64, 4), (127, 7), (64, 3), (124, 2), (67, 1), (127, 4))
KINDS = ("rough0", "nan_depth", "zero_normal", "sky")


def _frame(width, height, seed, **kw):
    """CSM + LPV with a sky bound over the atrium; roughness bytes >= 1, so that what the frame defers is what the test plants"""
    f = lc.MatrixFrame(width, height, flavour="atrium", seed=seed, shadowmap_res=128, **dict(lc.CSM_LPV, **kw))
    assert f.has_sky
    for k in ("color", "normals", "data", "emission", "depth"):
        f.arrays[k] = f.arrays[k].copy()
    f.arrays["data"][..., 1] = np.maximum(f.arrays["data"][..., 1], 1)
    return f


def _positions(width, r0, r1):
    """frame coordinates (x, y) of the planted pixels of a launch over rows [r0, r1)"""
    rows = r1 - r0
    out = [(x, r0 + y) for x, y in CORNERS if x < width and y < rows]
    # rows behind the last full band: rows % 4 at 4 pixels per thread, rows % 2 at 2 — the last rows of the launch cover both
    for back, x in ((1, 0), (1, 31), (1, 32), (2, width - 2), (3, 5), (4, 33), (5, 1), (5, width - 1)):
        if rows - back >= 0 and (x, r1 - back) not in out and 0 <= x < width:
            out.append((x, r1 - back))
    out.append((width - 2, r1 - 1))
    out.append((width - 1, r1 - 1))  # the last pixel
    seen, uniq = set(), []
    for p in out:
        if p not in seen and r0 <= p[1] < r1:
            seen.add(p)
            uniq.append(p)
    return uniq


def _plant(f, positions, shift=0, all_sky=False):
    """kinds in turn over the positions (`shift` rotates them); returns the number of planted pixels that are not sky.  `all_sky`: sky at every
    position — the frame whose deferred pixels are the ones the atrium itself has outside the planted positions."""
    n = 0
    for i, (x, y) in enumerate(positions):
        kind = "sky" if all_sky else KINDS[(i + shift) % len(KINDS)]
        if kind == "rough0":
            f.arrays["data"][y, x, 1] = 0
        elif kind == "nan_depth":
            f.arrays["depth"][y, x] = np.float32("nan")
        elif kind == "zero_normal":
            f.arrays["normals"][y, x, :3] = 0
        else:
            f.arrays["depth"][y, x] = 0.0
        if kind != "sky":
            # (a pixel the atrium left as sky would stay sky under a roughness or a normal edit)
            if f.arrays["depth"][y, x] == 0.0:
                f.arrays["depth"][y, x] = np.float32(0.5)
            n += 1
    return n


def _expected_tiled(width, rows, ppt):
    return width % 64 == 0 and rows >= ppt


def _run_paths(f, ctx, name, planted, background, r0=0, r1=None, ref=None):
    """every path over rows [r0, r1) of f: the image, the deferred count, the oracle"""
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
                want_ppt = lc.expected_ppt(f.width, r1 - r0, True, forced)
                assert rep["family"] == "fast" and rep["ppt"] == want_ppt and rep["sky_workgroups"] > 0, f"{name} [{path}]: {rep}"
                deferred = ctx.deferred_pixels()
                print(f"{name} [{path}]: ppt {rep['ppt']}, tiles {_expected_tiled(f.width, r1 - r0, rep['ppt'])}, {deferred} deferred pixels, "
                      f"{planted} planted, {background} of the frame's own")
                assert deferred == planted + background, f"{name} [{path}]: {deferred} pixels deferred, {planted} planted + {background} of the frame's own"
            d = util.f16_ulp_diff(got[r0:r1], ref[r0:r1])
            print(util.report_ulp(f"{name} [{path}]", d))
            assert d.max() <= MAX_ULP, util.report_ulp(f"{name} [{path}]", d)
            if not whole:
                assert not got[:r0].any() and not got[r1:].any(), f"{name} [{path}]: a row outside [{r0}, {r1}) was written"
            outs[path] = got
    finally:
        ctx.debug_set(force_general=False, force_ppt=0)
        f.row_begin = f.row_end = 0
    for path in outs:
        assert np.array_equal(outs[path], outs["general"]), f"{name}: the {path} path and the general kernel disagree"
    return outs


def _background(f_sky, ctx, r0, r1):
    """what the atrium itself defers outside the planted positions (those are sky in f_sky, and sky pixels are not listed): a property of the
    pixels, whatever the map"""
    whole = (r0, r1) == (0, f_sky.height)
    f_sky.row_begin, f_sky.row_end = (0, 0) if whole else (r0, r1)
    try:
        f_sky.run_hip(ctx)
        assert ctx.lighting_dispatch()["family"] == "fast"
        return ctx.deferred_pixels()
    finally:
        f_sky.row_begin = f_sky.row_end = 0


# (96 x 21 and 72 x 16: no whole 64-pixel tiles, the linear map; 128 x 21 and 128 x 23: one and three rows behind the last full band at 4 pixels per
# thread, one at 2)
SHAPES = [("64x16", 64, 16, 0, 16, None), ("96x21-linear", 96, 21, 0, 21, None), ("128x21", 128, 21, 0, 21, None), ("128x23", 128, 23, 0, 23, None),
          ("72x16-linear", 72, 16, 0, 16, None), ("64x24-rows3-19", 64, 24, 3, 19, None),
          ("64x16-pitched", 64, 16, 0, 16, {"color": dict(row_pad=16, offset=16), "normals": dict(row_pad=32, offset=32), "data": dict(row_pad=16),
                                            "emission": dict(row_pad=48, offset=16), "depth": dict(row_pad=16, offset=48), "ao": dict(row_pad=64, offset=16),
                                            "lit": dict(row_pad=32, offset=64)})]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_planted_pixels_land_where_they_belong(hip_ctx, shape):
    name, width, height, r0, r1, pitch = shape
    seed = 4100 + width + height
    positions = _positions(width, r0, r1)
    assert (width - 1, r1 - 1) in positions and (0, r0) in positions
    f = _frame(width, height, seed, pitch=pitch)
    planted = _plant(f, positions)
    assert planted >= 9 and len(positions) - planted >= 3, (planted, len(positions))
    f_sky = _frame(width, height, seed, pitch=pitch)
    _plant(f_sky, positions, all_sky=True)
    background = _background(f_sky, hip_ctx, r0, r1)
    _run_paths(f, hip_ctx, name, planted, background, r0, r1)
    # the other kinds at the same places
    g = _frame(width, height, seed, pitch=pitch)
    planted = _plant(g, positions, shift=2)
    _run_paths(g, hip_ctx, name + " (kinds rotated)", planted, background, r0, r1)


def test_kept_gather_copy_under_the_tile_map():
    """64 x 16 twice with the same lpv_generation: the second call gathers from the copy the first one built"""
    import torch
    from androidrenderer_amd import lib
    ctx = lib.Context(device=0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        positions = _positions(64, 0, 16)
        f = _frame(64, 16, 4180)
        planted = _plant(f, positions)
        f_sky = _frame(64, 16, 4180)
        _plant(f_sky, positions, all_sky=True)
        background = _background(f_sky, ctx, 0, 16)
        f.lpv_generation = 23
        ref = f.run_oracle()
        dev = f.device_arrays()
        ctx.debug_set(force_ppt=4)
        packs = ctx.copy_rebuilds()[0]
        outs = []
        for call in (0, 1):
            got = f.run_hip(ctx, dev)
            rep = ctx.lighting_dispatch()
            assert rep["family"] == "fast" and rep["ppt"] == 4 and rep["repack"] == (1 if call == 0 else 0), (call, rep)
            assert ctx.deferred_pixels() == planted + background
            d = util.f16_ulp_diff(got, ref)
            assert d.max() <= MAX_ULP, util.report_ulp(f"call {call}", d)
            outs.append(got)
        assert ctx.copy_rebuilds()[0] == packs + 1, "the LPV gather copy was rebuilt although lpv_generation stood"
        assert np.array_equal(outs[0], outs[1])
        ctx.debug_set(force_general=True)
        assert np.array_equal(f.run_hip(ctx, dev), outs[0]), "the fast path and the general kernel disagree"
    finally:
        ctx.debug_set()
        torch.cuda.synchronize()
        ctx.close()
