"""GPU parity matrix of the Lighting pass over the uniform blocks: cameras, suns, LPV layouts, plane pitches, extents, row ranges and state
across calls (tests/lighting_cases.py is the case list; tests/test_lighting_matrix_cpu.py checks with the oracle alone that every case shades
what it claims to).  tests/test_lighting_gpu.py is thorough in the pixels but holds the uniform blocks at one point — the very thing the fast
path's proofs (api.cpp: detect_fast_path) quantify over.

Bars, the project's own: every device path bit-equal to the general kernel, every path within MAX_ULP = 1 of the oracle (BASELINE.json
north_star).  Every case also asserts the kernel branch it claims to test, from the library's dispatch report (lib.Context.lighting_dispatch):
a case cannot slide onto another branch unnoticed — as the whole suite has with pos_div_nr, which SceneView.default never enables (its inverse
projection has -0.0 where the proof needs +0)."""
import time

import numpy as np
import pytest

from tests import lighting_cases as lc
from tests import util

pytestmark = pytest.mark.gpu

MAX_ULP = util.MAX_ULP

PATHS = (("auto", False, 0), ("4 px per thread", False, 4), ("2 px per thread", False, 2), ("general", True, 0))


def _expected_launch(width, rows, ppt, has_sky):
    """row_magic / sky_ratio / leading sky workgroups of a fast-kernel launch, restated from the rules DESIGN.md §7 gives for them"""
    gpr = width // ppt
    blocks = (gpr * rows + 255) // 256
    threads = blocks * 256
    ratio = min(max((blocks + 511) // 512, 4), 32)
    return {"row_magic": int(gpr >= 2 and threads * gpr < 2 ** 32), "sky_ratio": ratio, "sky_workgroups": (blocks + ratio - 1) // ratio if has_sky else 0}


def _assert_report(rep, f, expect, vec4, general, forced, rows, name):
    lights = f.lights is not None
    if general:
        want = {"family": "tiled", "tiled_fast_geom": 0, "tiled_fast_lpv": 0} if lights else {"family": "general"}
    else:
        want = dict(expect)
    if want["family"] != "tiled":
        want["ppt"] = lc.expected_ppt(f.width, rows, vec4, forced)
    if want["family"] == "fast":
        want.update(_expected_launch(f.width, rows, want["ppt"], f.has_sky))
    got = {k: rep[k] for k in want}
    assert got == want, f"{name}: the call took another branch than the case names: {rep}"


def _assert_deferred(ctx, rep, pixels, name):
    """After a fast-family call: at most a quarter of the call's pixels went to the fix-up kernel (the share test_lpv_generation... uses) — a fast
    kernel that hands everything to the fix-up is bit-equal to the general kernel and not being tested.  Sky pixels are not counted."""
    if rep["family"] != "fast":
        return
    deferred = ctx.deferred_pixels()
    print(f"{name}: {rep}, {deferred} deferred pixels of {pixels}")
    assert deferred <= pixels // 4, f"{name}: {deferred} of {pixels} pixels deferred"


def _check(f, ctx, name, expect, vec4=True, exempt=None, paths=PATHS, ref=None):
    """The paths of tests/test_lighting_gpu.py's _check — automatic, forced 4 / 2 pixels per thread, general — each on the branch `expect` names,
    within MAX_ULP of the oracle and bit-equal to the general kernel."""
    ref = f.run_oracle() if ref is None else ref
    dev = f.device_arrays()
    outs = {}
    try:
        for path, general, forced in paths:
            ctx.debug_set(force_general=general, force_ppt=forced)
            got = f.run_hip(ctx, dev)
            rep = ctx.lighting_dispatch()
            _assert_report(rep, f, expect, vec4, general, forced, f.height, f"{name} [{path}]")
            if exempt is None:
                _assert_deferred(ctx, rep, f.width * f.height, f"{name} [{path}]")
            else:
                print(f"{name} [{path}]: {rep} (no deferred-pixel cap: {exempt})")
            outs[path] = got
            d = util.f16_ulp_diff(got, ref)
            print(util.report_ulp(f"{name} [{path}]", d))
            assert d.max() <= MAX_ULP, util.report_ulp(f"{name} [{path}]", d)
    finally:
        ctx.debug_set(force_general=False, force_ppt=0)
    for path in outs:
        assert np.array_equal(outs[path], outs["general"]), f"{name}: the {path} path and the general kernel disagree"
    return outs


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_parity_matrix(hip_ctx, case):
    f = case.build()
    ref = f.run_oracle()
    if case.nonfinite:  # (the vertical sun: NaN cascade matrices, NaN placement identical to the oracle — f16_ulp_diff counts NaN against a number as 65535)
        assert float(((ref[..., :3] & 0x7C00) == 0x7C00).any(-1).mean()) >= case.nonfinite
    _check(f, hip_ctx, case.name, case.expect, vec4=case.vec4, exempt=case.exempt, ref=ref)


def test_pos_div_nr_is_on_only_where_a_case_sets_plus_zero(hip_ctx):
    """The shared-reciprocal divide (lighting_fast.hpp: fast_geometry) is reached by the plus_zero cases and by nothing else of the matrix; the
    same frame with -0.0 in either entry stays on the IEEE divides (with a -0 addend the numerators can become -0, outside the divide's proof)."""
    f = lc.BY_NAME["camera-plus_zero-csm_lpv-atrium"].build()
    dev = f.device_arrays()
    for p12, p13, want in ((0.0, 0.0, 1), (-0.0, -0.0, 0), (0.0, -0.0, 0), (-0.0, 0.0, 0)):
        f.view.gpu_data.inverse_projection[12] = p12
        f.view.gpu_data.inverse_projection[13] = p13
        got = f.run_hip(hip_ctx, dev)
        rep = hip_ctx.lighting_dispatch()
        assert rep["family"] == "fast" and rep["pos_div_nr"] == want, (p12, p13, rep)
        _assert_deferred(hip_ctx, rep, f.width * f.height, f"inverse_projection[12], [13] = {p12}, {p13}")
        d = util.f16_ulp_diff(got, f.run_oracle())
        assert d.max() <= MAX_ULP, util.report_ulp(f"inverse_projection[12], [13] = {p12}, {p13}", d)


@pytest.mark.parametrize("row", [0, 71, 143])
def test_one_row_ranges(hip_ctx, row):
    """A row range of one row at the top, in the middle and at the bottom: that row as the whole frame has it, every other row untouched."""
    import torch
    f = lc.MatrixFrame(256, 144, flavour="random", seed=700, **lc.CSM_LPV)
    ref = f.run_oracle()
    dev = f.device_arrays()
    f.row_begin, f.row_end = row, row + 1
    outs = {}
    try:
        for path, general, forced in PATHS:
            hip_ctx.debug_set(force_general=general, force_ppt=forced)
            lit = torch.full((144, 256, 4), 0x2525, dtype=torch.int16, device="cuda")
            d, keep = f.describe(dev, lit)
            hip_ctx.lighting(d)
            torch.cuda.synchronize()
            rep = hip_ctx.lighting_dispatch()
            _assert_report(rep, f, dict(lc.FAST, ncasc_pow2=1), True, general, forced, 1, f"row {row} [{path}]")
            _assert_deferred(hip_ctx, rep, 256, f"row {row} [{path}]")
            got = util.from_torch(lit, np.uint16)
            outside = np.ones(144, bool)
            outside[row] = False
            assert (got[outside] == 0x2525).all(), f"row {row} [{path}]: a row outside the range was written"
            assert util.f16_ulp_diff(got[row], ref[row]).max() <= MAX_ULP
            outs[path] = got
    finally:
        hip_ctx.debug_set(force_general=False, force_ppt=0)
    for path in outs:
        assert np.array_equal(outs[path], outs["general"])


def test_one_group_per_row_has_no_row_magic(hip_ctx):
    """W / ppt == 1: the multiply-high row split needs two groups per row (magic = floor(2^32 / d) + 1 does not fit 32 bits for d = 1)"""
    for name, forced in (("extent-4x45", 4), ("extent-2x45", 1), ("extent-1x45", 1)):
        f = lc.BY_NAME[name].build()
        hip_ctx.debug_set(force_ppt=forced)
        try:
            got = f.run_hip(hip_ctx)
            rep = hip_ctx.lighting_dispatch()
        finally:
            hip_ctx.debug_set()
        assert rep["family"] == "fast" and rep["ppt"] == forced and rep["row_magic"] == (1 if f.width // forced >= 2 else 0), rep
        _assert_deferred(hip_ctx, rep, f.width * f.height, name)
        assert util.f16_ulp_diff(got, f.run_oracle()).max() <= MAX_ULP


@pytest.mark.parametrize("flavour", ["atrium", "random"])
@pytest.mark.parametrize("height", lc.BIG_HEIGHTS)
def test_launch_geometry_edges(hip_ctx, height, flavour):
    """Launch geometry that small frames never reach, against the oracle over the WHOLE frame (the full-size tests compare three 8-row bands):
    3,840 groups per row at one pixel per thread put threads * groups-per-row at 4.29e9 < 2^32 for 291 rows and 4.31e9 >= 2^32 for 292 — either
    side of the multiply-high row split's limit — and 4,365 / 4,380 workgroups give sky_ratio 9, between the 4 of every small test and the
    16 / 32 of 4K / 8K.  Then the frame as three row shards, which pick one pixel per thread and sky_ratio 4 where the whole frame picks 2 and 5."""
    import torch
    f = lc.big_frame(height, flavour)
    t0 = time.perf_counter()
    ref = f.run_oracle()
    print(f"oracle, 3840 x {height} {flavour}: {time.perf_counter() - t0:.2f} s")
    dev = f.device_arrays()
    exp = dict(lc.FAST, ncasc_pow2=1)
    outs = {}
    try:
        for path, general, forced in PATHS + (("1 px per thread", False, 1),):
            hip_ctx.debug_set(force_general=general, force_ppt=forced)
            got = f.run_hip(hip_ctx, dev)
            rep = hip_ctx.lighting_dispatch()
            print(f"3840 x {height} {flavour} [{path}]: {rep}")
            _assert_report(rep, f, exp, True, general, forced, height, path)
            if forced == 1:  # stated outright, not through the restated rule
                assert (rep["ppt"], rep["row_magic"], rep["sky_ratio"]) == (1, 1 if height == 291 else 0, 9), rep
            if path == "auto":
                assert (rep["ppt"], rep["row_magic"], rep["sky_ratio"]) == (2, 1, 5), rep
            _assert_deferred(hip_ctx, rep, 3840 * height, f"3840 x {height} {flavour} [{path}]")
            d = util.f16_ulp_diff(got, ref)
            print(util.report_ulp(f"3840 x {height} {flavour} [{path}]", d))
            assert d.max() <= MAX_ULP, util.report_ulp(path, d)
            outs[path] = got
    finally:
        hip_ctx.debug_set(force_general=False, force_ppt=0)
    for path in outs:
        assert np.array_equal(outs[path], outs["general"]), f"the {path} path and the general kernel disagree"
    lit = torch.zeros((height, 3840, 4), dtype=torch.int16, device="cuda")
    for r0, r1 in lc.BIG_SHARDS:
        f.row_begin, f.row_end = r0, (height if r1 is None else r1)
        d, keep = f.describe(dev, lit)
        hip_ctx.lighting(d)
        rep = hip_ctx.lighting_dispatch()
        print(f"rows [{f.row_begin}, {f.row_end}): {rep}")
        # every shard: 97 / 103 / 91-92 rows of 3,840 pixels are fewer than 1,536 workgroups even at one pixel per thread
        assert (rep["family"], rep["ppt"], rep["row_magic"], rep["sky_ratio"]) == ("fast", 1, 1, 4), rep
        _assert_deferred(hip_ctx, rep, 3840 * (f.row_end - f.row_begin), f"rows [{f.row_begin}, {f.row_end})")
    torch.cuda.synchronize()
    assert np.array_equal(util.from_torch(lit, np.uint16), outs["auto"]), "the three row shards differ from the unsharded image"


# ---- state across calls ------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def fresh_ctx():
    """a context of its own: the tests below count what the context rebuilt since it was made"""
    import torch
    from androidrenderer_amd import lib
    ctx = lib.Context(device=0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    yield ctx
    torch.cuda.synchronize()
    ctx.close()


@pytest.mark.parametrize("lights", [0, 24], ids=["fast", "tiled"])
def test_empty_row_range_does_not_claim_the_lpv_copy(fresh_ctx, lights):
    """A shard plan can hand a rank no rows (row_begin == row_end != 0).  Such a call launches nothing, so it must not record the gather copy of
    the LPV volumes as built: the next call with the same lpv_generation would gather from a copy that was never made.  Both kernels that gather
    from the copy — the fast one and the tiled one with the fast LPV overlay — guard their bookkeeping with `r1 > r0` (api.cpp)."""
    ctx = fresh_ctx
    kw = dict(lights=lc.synth.point_lights(lc.make_view(256, 144), lights, 6.0, seed=801)) if lights else {}
    f = lc.MatrixFrame(256, 144, flavour="atrium", seed=710, **dict(lc.CSM_LPV, **kw))
    f.lpv_generation = 7
    dev = f.device_arrays()
    want = f.run_oracle()
    before = ctx.copy_rebuilds()[0]
    f.row_begin = f.row_end = 5
    import torch
    lit = torch.full((144, 256, 4), 0x2525, dtype=torch.int16, device="cuda")
    d, keep = f.describe(dev, lit)
    ctx.lighting(d)
    torch.cuda.synchronize()
    assert bool((lit == 0x2525).all()), "an empty row range wrote pixels"
    assert ctx.copy_rebuilds()[0] == before, "an empty row range claimed to have rebuilt the gather copy"
    f.row_begin = f.row_end = 0
    got = f.run_hip(ctx, dev)
    rep = ctx.lighting_dispatch()
    assert rep["family"] == ("tiled" if lights else "fast") and rep["repack"] == 1 and (not lights or rep["tiled_fast_lpv"] == 1), rep
    _assert_deferred(ctx, rep, 256 * 144, "full frame after an empty row range")
    assert ctx.copy_rebuilds()[0] == before + 1, "the pack kernel did not run for the first call that shades pixels"
    d = util.f16_ulp_diff(got, want)
    assert d.max() <= MAX_ULP, util.report_ulp("full frame after an empty row range", d)
    again = f.run_hip(ctx, dev)  # ... and the copy is kept from then on
    assert ctx.lighting_dispatch()["repack"] == 0 and ctx.copy_rebuilds()[0] == before + 1 and np.array_equal(again, got)


@pytest.mark.parametrize("lights", [0, 24], ids=["fast", "tiled"])
def test_camera_change_rebuilds_the_column_table(fresh_ctx, lights):
    """The column / row table of view-space numerators is keyed on {render resolution, p0, p12, p5, p13, H}: default -> jitter -> +0 -> default at
    one extent and under a kept LPV copy rebuilds it four times (+0 and -0 are different keys), the same camera twice does not; every image
    against its oracle.  The fast kernel reads the table at 4 pixels per thread, the tiled kernel whenever it borrows the fast geometry."""
    ctx = fresh_ctx
    kw = dict(lights=lc.synth.point_lights(lc.make_view(256, 144), lights, 6.0, seed=802)) if lights else {}
    f = lc.MatrixFrame(256, 144, flavour="random", seed=720, **dict(lc.CSM_LPV, **kw))
    f.lpv_generation = 11
    dev = f.device_arrays()
    walk = ("default", "jitter", "plus_zero", "default")
    if not lights:
        ctx.debug_set(force_ppt=4)
    packs = ctx.copy_rebuilds()[0]
    for k, cam in enumerate(walk):
        f.set_camera(regenerate=False, **lc.CAMERAS[cam])  # (the same G-buffer and volumes; cascades and LPV transforms refitted)
        want = f.run_oracle()
        for repeat in (0, 1):
            got = f.run_hip(ctx, dev)
            rep = ctx.lighting_dispatch()
            print(f"{cam} (call {repeat}): {rep}")
            assert rep["family"] == ("tiled" if lights else "fast") and rep["table_rebuilt"] == (1 if repeat == 0 else 0), (cam, repeat, rep)
            _assert_deferred(ctx, rep, 256 * 144, f"camera {cam}, call {repeat}")
            assert rep["pos_div_nr"] == (1 if cam == "plus_zero" else 0) and rep["repack"] == (1 if k == 0 and repeat == 0 else 0), (cam, repeat, rep)
            if lights:
                assert rep["tiled_fast_geom"] == 1 and rep["tiled_fast_lpv"] == 1, rep
            else:
                assert rep["ppt"] == 4, rep
            d = util.f16_ulp_diff(got, want)
            assert d.max() <= MAX_ULP, util.report_ulp(f"camera {cam}, call {repeat}", d)
    assert ctx.copy_rebuilds()[0] == packs + 1, "the LPV gather copy was rebuilt although lpv_generation stood"
    ctx.debug_set()
