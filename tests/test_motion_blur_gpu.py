"""GPU: sah_motion_blur (include/sah_motion_blur.h) against the numpy restatement (tests/motion_blur_ref.py) run on the device's own planes,
and its committed fixture, bit for bit: extents one below, at and one above the 16 x 16 tile and workgroup in each axis; tap counts, dither,
the clamp and the pass-through threshold; vectors that leave every border; the property cases of tests/test_motion_blur_cpu.py on the
device; the upscale; row windows; pitches, offsets and alignment; the invariants; stream capture, the refusals and frame.MotionBlur over
three frames of a panning camera on the rasterised atrium."""
import faulthandler
import math
import os
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, lib, mesh, scene
from tests import layouts
from tests import motion_blur_ref as ref
from tests import util
from tests.support import context_state, differs, Image, resized, retyped, same, SENTINEL, side_stream_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_motion_blur as gen  # noqa: E402

f32 = np.float32
RGBA16, RG16, D32 = _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R16G16_SFLOAT, _abi.FORMAT_D32_SFLOAT
FORMATS = dict(scene=RGBA16, depth=D32, mv=RG16, tiles=RG16, out=RGBA16)
ORDER = ("scene", "depth", "mv", "tiles", "out")
INPUTS = ORDER[:3]
EXTENTS = [(15, 17), (16, 16), (33, 31), (47, 49), (96, 54)]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)  # each test under a limit of its own: an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fixture():
    fx = np.load(gen.FIXTURE)
    return {k: fx[k] for k in fx.files}


def _params(**changes):
    return _abi.MotionBlurParams.default(**changes)


class Planes:
    """the five device planes of one call; pitches / offsets by plane name"""

    def __init__(self, scene_bits, depth, mv, pitches=None, offsets=None):
        self.H, self.W = scene_bits.shape[:2]
        self.h, self.w = depth.shape
        pitches, offsets = pitches or {}, offsets or {}
        extent = dict(scene=(self.W, self.H), out=(self.W, self.H), depth=(self.w, self.h), mv=(self.w, self.h),
                      tiles=((self.w + 15) // 16, (self.h + 15) // 16))
        data = dict(scene=scene_bits, depth=depth, mv=mv)
        self.img = {n: Image(FORMATS[n], *extent[n], pitches.get(n), data.get(n), offsets.get(n, 0)) for n in ORDER}
        self.out = self.img["out"]

    def planes(self):
        return [self.img[n].plane for n in ORDER]

    def result(self):
        return self.out.texels(np.uint16).reshape(self.H, self.W, 4)

    def tiles(self):
        return self.img["tiles"].texels(np.uint16).reshape(self.img["tiles"].h, self.img["tiles"].w, 2)

    def run(self, ctx, params, rows=(0, 0)):
        import torch
        ctx.motion_blur(*self.planes(), params, rows)
        torch.cuda.synchronize()
        assert all(self.img[n].unchanged() for n in INPUTS), "an input changed"
        assert self.img["tiles"].padding_intact() and (rows != (0, 0) or self.out.padding_intact())  # (a windowed caller checks the other rows itself)
        return self.result()


def _check(hip_ctx, scene_bits, depth, mv, settings, **kw):
    """one whole-frame call against the restatement, the tile plane included; -> (got, info)"""
    p = Planes(scene_bits, depth, mv, **kw)
    got = p.run(hip_ctx, _params(**settings))
    want, info = ref.motion_blur_ex(scene_bits, depth, mv, **settings)
    assert same(p.tiles(), info["tiles"]), f"{settings}: tiles " + differs(p.tiles(), info["tiles"])
    assert same(got, want), f"{settings}: " + differs(got, want)
    return got, info


def _random_field(w, h, seed, sigma=12.0, W=None, H=None):
    """a textured scene over a box-and-wall depth with holes, and vectors of every length around the threshold and the cap"""
    g = np.random.default_rng(seed)
    depth = ref.box_depth(w, h).copy()
    depth[g.random((h, w)) < 0.05] = 0.0
    mv = g.normal(0.0, sigma, (h, w, 2)) * (g.random((h, w, 1)) < 0.3)  # most texels still: tiles of every mixture
    return ref.textured_scene(W or w, H or h, seed), depth, ref.to_half_bits(mv)


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(gen.CASES)))
def test_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture, case):
    field, settings = gen.CASES[case]
    p = Planes(fixture["scene"], fixture[f"{field}_depth"], fixture[f"{field}_mv"])
    got = p.run(hip_ctx, _params(**settings))
    assert same(got, fixture["out"][case]), differs(got, fixture["out"][case])
    again = p.run(hip_ctx, _params(**settings))  # two calls, the same bytes
    assert same(again, got)


# ---- extents and parameters ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: f"{e[0]}x{e[1]}")
def test_parity_over_extents_tap_counts_and_dither(hip_ctx, extent):
    w, h = extent
    scene_bits, depth, mv = _random_field(w, h, 100 + w)
    blurred = 0
    for settings in (dict(), dict(sample_count=2), dict(sample_count=32, flags=ref.DITHER), dict(flags=ref.DITHER, shutter=1.0, depth_extent=0.3)):
        _, info = _check(hip_ctx, scene_bits, depth, mv, settings)
        blurred += int((~info["passed"]).sum())
    assert blurred


def test_vectors_longer_than_the_cap_and_speeds_around_the_threshold(hip_ctx):
    w, h = 47, 49
    g = np.random.default_rng(5)
    scene_bits = ref.textured_scene(w, h, 5)
    depth = ref.box_depth(w, h)
    long = ref.to_half_bits(g.normal(0.0, 150.0, (h, w, 2)))  # scaled by the shutter: far beyond 32
    _, info = _check(hip_ctx, scene_bits, depth, long, dict(max_blur_pixels=32.0))
    assert (info["speed"] == 32.0).all() and not info["passed"].all()
    _check(hip_ctx, scene_bits, depth, long, dict(max_blur_pixels=5.5, shutter=1.0))
    # four lone movers in the corner tiles of a 6 x 4 grid, their scaled lengths around min_velocity_pixels = 0.5: 0.4 and 0.49 pass through,
    # 0.5 itself (not shorter) and 0.6 blur, each with the tiles around it
    w, h = 96, 54
    scene_bits, depth = ref.textured_scene(w, h, 6), ref.box_depth(w, h)
    slow = np.zeros((h, w, 2), f32)
    slow[3, 5], slow[2, 90], slow[50, 4], slow[52, 93] = (0.8, 0.0), (0.0, 1.2), (-1.0, 0.0), (0.0, -0.98)
    _, info = _check(hip_ctx, scene_bits, depth, ref.to_half_bits(slow), dict(min_velocity_pixels=0.5))
    assert not info["moving"][:32, :32].any() and info["moving"][:32, 64:].all() and info["moving"][32:, :32].all() and not info["moving"][32:, 64:].any()
    assert not info["passed"].all()
    for min_velocity in (0.0, 0.45, 0.55):
        _check(hip_ctx, scene_bits, depth, ref.to_half_bits(slow), dict(min_velocity_pixels=min_velocity))


@pytest.mark.parametrize("vector", [(-90.0, 0.0), (90.0, 0.0), (0.0, -90.0), (0.0, 90.0), (70.0, 70.0), (-70.0, -70.0)])
def test_vectors_that_point_off_every_border(hip_ctx, vector):
    w, h = 33, 31
    _, info = _check(hip_ctx, ref.textured_scene(w, h, 9), ref.box_depth(w, h), ref.pan_vectors(w, h, vector), dict(shutter=1.0, sample_count=32))
    assert not info["passed"].all()


# ---- the property cases of the CPU test, on the device -----------------------------------------------------------------------------------
def test_static_foreground_keeps_its_bytes_on_the_device(hip_ctx):
    w, h = gen.WIDTH, gen.HEIGHT
    scene_bits, depth, box = ref.textured_scene(w, h, 4), ref.box_depth(w, h), ref.box_mask(w, h)
    mv = ref.to_half_bits(np.where(box[..., None], 0.0, np.array([18.0, 10.0])))
    got, info = _check(hip_ctx, scene_bits, depth, mv, dict())
    assert (got[box] == scene_bits[box]).all() and info["moving"].all() and (got[~box] != scene_bits[~box]).any()


def test_a_mover_in_the_diagonal_tile_on_the_device(hip_ctx):
    w, h = 48, 40
    scene_bits, depth = ref.textured_scene(w, h, 6), np.full((h, w), 0.01, f32)
    mv = np.zeros((h, w, 2), f32)
    mv[16, 16] = (-64.0, -64.0)
    got, _ = _check(hip_ctx, scene_bits, depth, ref.to_half_bits(mv), dict(sample_count=32))
    assert (got[5, 5] != scene_bits[5, 5]).any()


def test_the_tie_rule_on_the_device(hip_ctx):
    g = np.random.default_rng(7)
    w, h = 48, 33
    mv = ref.to_half_bits(np.round(g.normal(0.0, 3.0, (h, w, 2))))  # small integers: many exact ties within a tile and between tiles
    _check(hip_ctx, ref.textured_scene(w, h, 7), ref.box_depth(w, h), mv, dict(shutter=1.0))
    one = np.zeros((16, 16, 2), f32)
    one[2, 3], one[11, 9] = (3.0, 4.0), (-4.0, 3.0)
    p = Planes(ref.textured_scene(16, 16, 7), ref.box_depth(16, 16), ref.to_half_bits(one))
    p.run(hip_ctx, _params())
    assert int(ref.pair_bits(p.tiles())[0, 0]) == max(int(ref.pair_bits(ref.to_half_bits(np.array(v, f32)))) for v in ((3.0, 4.0), (-4.0, 3.0)))


def test_non_finite_vectors_and_unclean_texels_on_the_device(hip_ctx):
    w, h = 48, 40
    scene_bits, depth = ref.textured_scene(w, h, 8), ref.box_depth(w, h).copy()
    mv = ref.pan_vectors(w, h, (14.0, 6.0)).copy()
    for k, bits in enumerate((0x7E00, 0x7C00, 0xFC00, 0xFE00)):
        mv[5 + k, 7, k & 1] = bits
    for (x, y, c, bits) in ((20, 12, 0, 0x7E00), (21, 30, 1, 0x7C00), (33, 17, 2, 0xBC00), (40, 25, 0, 0xFC00)):
        scene_bits[y, x, c] = bits
    depth[::3, ::2], depth[1::3, 1::2], depth[2::5, ::3], depth[::7, 1::3] = 0.0, np.nan, np.inf, -1.0
    got, _ = _check(hip_ctx, scene_bits, depth, mv, dict())
    assert (~ref.clean(ref.h2f(got[..., :3]))).sum() == 4
    for bits in (0x7E00, 0x7C00, 0xFC00):
        got, _ = _check(hip_ctx, scene_bits, depth, np.full((h, w, 2), bits, np.uint16), dict())
        assert same(got, scene_bits)


def test_a_static_camera_copies_the_scene_on_either_path(hip_ctx):
    w, h = 47, 49
    jitter, previous = (0.25, -0.375), (-0.125, 0.3125)
    scene_bits, depth = ref.textured_scene(w, h, 11), ref.box_depth(w, h)
    mv = ref.static_vectors(w, h, jitter, previous)
    for kw in (dict(), dict(offsets=dict(scene=8, out=4))):
        got, _ = _check(hip_ctx, scene_bits, depth, mv, dict(jitter=jitter, previous_jitter=previous), **kw)
        assert same(got, scene_bits)


# ---- upscale ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("render,output", [((64, 36), (96, 54)), ((40, 31), (47, 49)), ((33, 17), (33, 31))], ids=["1.5x", "unequal", "y-only"])
def test_upscale(hip_ctx, render, output):
    (w, h), (W, H) = render, output
    scene_bits, depth, mv = _random_field(w, h, 31 + w, W=W, H=H)
    for settings in (dict(), dict(flags=ref.DITHER, jitter=(0.25, -0.375), previous_jitter=(-0.125, 0.3125), sample_count=8)):
        _, info = _check(hip_ctx, scene_bits, depth, mv, settings)
        assert not info["passed"].all()


# ---- row windows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("render,output", [((47, 49), (47, 49)), ((40, 31), (47, 49))], ids=["equal", "upscale"])
def test_row_windows_cover_the_frame_and_write_nothing_else(hip_ctx, render, output):
    import torch
    (w, h), (W, H) = render, output
    scene_bits, depth, mv = _random_field(w, h, 41, W=W, H=H)
    settings = dict(flags=ref.DITHER, jitter=(0.25, 0.125), previous_jitter=(0.0, 0.0))
    want = ref.motion_blur(scene_bits, depth, mv, **settings)
    whole = Planes(scene_bits, depth, mv).run(hip_ctx, _params(**settings))
    assert same(whole, want)
    banded = Planes(scene_bits, depth, mv)
    for rows in ((0, 7), (7, 8), (8, 24), (24, 24), (24, 40), (40, H)):  # windows that split tile rows; a one-row and an empty window
        before = banded.result().copy()
        single = Planes(scene_bits, depth, mv)
        got = single.run(hip_ctx, _params(**settings), rows)
        assert same(got[rows[0]:rows[1]], want[rows[0]:rows[1]]), f"rows {rows}: " + differs(got[rows[0]:rows[1]], want[rows[0]:rows[1]])
        layouts.assert_rows_untouched(np.uint16(SENTINEL * 0x101), got, rows[0], rows[1], what=f"rows {rows}")
        if rows[0] == rows[1]:
            assert single.img["tiles"].unchanged()  # an empty band writes nothing at all
        banded.run(hip_ctx, _params(**settings), rows)
        layouts.assert_rows_untouched(before, banded.result(), rows[0], rows[1], what=f"rows {rows} of the union")
    torch.cuda.synchronize()
    assert same(banded.result(), whole)


# ---- layout -------------------------------------------------------------------------------------------------------------------------------
def test_pitched_offset_and_misaligned_planes_give_the_same_bytes(hip_ctx):
    w, h = 47, 49
    scene_bits, depth, mv = _random_field(w, h, 51)
    settings = dict(flags=ref.DITHER)
    tight, _ = _check(hip_ctx, scene_bits, depth, mv, settings)  # torch allocations: 16-byte aligned, the wide path
    # 4-byte aligned planes against 16-byte aligned ones; pitches that are multiples of 16 with a base that is not, and the reverse
    for kw in (dict(offsets=dict(scene=4)), dict(offsets=dict(out=8)), dict(offsets=dict(mv=4, depth=12, tiles=4)),
               dict(pitches=dict(scene=w * 8 + 16, out=w * 8 + 32, mv=w * 4 + 4, depth=w * 4 + 12, tiles=3 * 4 + 8)),
               dict(pitches=dict(scene=w * 8 + 4, out=w * 8 + 12), offsets=dict(scene=16, out=16))):
        got, _ = _check(hip_ctx, scene_bits, depth, mv, settings, **kw)
        assert same(got, tight), kw


@pytest.mark.parametrize("spec", [dict(row_pad=8, offset=8), dict(row_pad=40, offset=16)], ids=["A", "B"])
def test_layouts_of_tests_layouts(hip_ctx, spec):
    """the two families of tests/layouts.py: the smallest padding and offset the argument check admits, and a padding that is a multiple of
    the texel but not of 16 — same bytes as the tight run, no padding byte written, inputs unchanged"""
    import torch
    w, h = 33, 31
    scene_bits, depth, mv = _random_field(w, h, 61)
    want = ref.motion_blur(scene_bits, depth, mv)
    arrays = dict(scene=util.to_torch(scene_bits), depth=torch.from_numpy(depth).cuda(), mv=util.to_torch(mv),
                  tiles=torch.full((2, 3, 2), 0x5A5A, dtype=torch.int16, device="cuda"), out=torch.full((h, w, 4), 0x5A5A, dtype=torch.int16, device="cuda"))
    small = dict(row_pad=spec["row_pad"] // 2, offset=spec["offset"] // 2)  # the 4-byte texels
    wrapped = layouts.wrap(arrays, {n: (FORMATS[n], 2) for n in ORDER}, dict(scene=spec, out=spec, depth=small, mv=small, tiles=small))
    hip_ctx.motion_blur(*[wrapped[n].plane() for n in ORDER], _params())
    torch.cuda.synchronize()
    assert same(wrapped["out"].read(np.uint16), want)
    layouts.assert_padding_intact(wrapped, what=str(spec))
    layouts.assert_inputs_unchanged({n: wrapped[n] for n in INPUTS}, what=str(spec))


# ---- runtime ------------------------------------------------------------------------------------------------------------------------------
def test_side_stream_under_capture_and_replayed_over_other_inputs(fixture):
    import torch
    fx = fixture
    field, settings = gen.CASES[2]
    with side_stream_context() as (ctx, s):
        a = Planes(fx["scene"], fx[f"{field}_depth"], fx[f"{field}_mv"])
        params = _params(**settings)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.motion_blur(*a.planes(), params)
        s.synchronize()
        assert same(a.result(), fx["out"][2])
        b = Planes(ref.textured_scene(gen.WIDTH, gen.HEIGHT, 71), fx["box_pan_depth"], fx["box_pan_mv"])
        direct = ref.motion_blur(b.img["scene"].texels(np.uint16).reshape(gen.HEIGHT, gen.WIDTH, 4), fx["box_pan_depth"], fx["box_pan_mv"], **settings)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.motion_blur(*a.planes(), params)
        for n in INPUTS:
            a.img[n].t.copy_(b.img[n].t)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same(a.result(), direct) and not same(direct, fx["out"][2])


def test_no_side_effects_on_the_context(hip_ctx, fixture):
    f = util.LightingFrame(64, 36, seed=5, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flavour="atrium")
    f.run_hip(hip_ctx)

    def state():
        return context_state(hip_ctx)
    before = state()
    got = Planes(fixture["scene"], fixture["dolly_depth"], fixture["dolly_mv"]).run(hip_ctx, _params())
    assert state() == before and same(got, fixture["out"][2])


def test_refusals_launch_nothing(hip_ctx, fixture):
    """(tests/test_motion_blur_cpu.py runs the whole list on a context without a device; here: the targets keep their bytes)"""
    import torch
    p = Planes(fixture["scene"], fixture["low_depth"], fixture["low_mv"])
    scene_p, depth, mv, tiles, out = p.planes()
    ok = _params()

    INVALID, FORMAT = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
    nan = float("nan")
    cases = [((scene_p, depth, mv, tiles, retyped(out, _abi.FORMAT_R32_SFLOAT), ok), FORMAT),
             ((scene_p, retyped(depth, _abi.FORMAT_R32_SFLOAT), mv, tiles, out, ok), FORMAT),
             ((scene_p, depth, mv, retyped(tiles, _abi.FORMAT_R32_SFLOAT), out, ok), FORMAT),
             ((scene_p, depth, mv, tiles, out, ok, (0, gen.HEIGHT + 1)), INVALID),
             ((scene_p, depth, mv, tiles, out, ok, (9, 3)), INVALID),
             ((scene_p, depth, mv, resized(tiles, 6, 4), out, ok), INVALID),                        # the output's tile grid, not the render raster's
             ((scene_p, resized(depth, 63, 36), mv, tiles, out, ok), INVALID),                      # the render planes differ
             ((resized(scene_p, 60, 54), depth, mv, tiles, resized(out, 60, 54), ok), INVALID),     # downscaling in x
             ((resized(scene_p, 96, 30), depth, mv, tiles, resized(out, 96, 30), ok), INVALID),     # downscaling in y
             ((scene_p, depth, mv, tiles, scene_p, ok), INVALID),                                   # in place
             ((scene_p, depth, mv, mv, out, ok), INVALID),                                          # tiles over an input (also the wrong extent)
             ((scene_p, depth, mv, tiles, out, _params(sample_count=13)), INVALID),
             ((scene_p, depth, mv, tiles, out, _params(sample_count=34)), INVALID),
             ((scene_p, depth, mv, tiles, out, _params(shutter=0.0)), INVALID),
             ((scene_p, depth, mv, tiles, out, _params(max_blur_pixels=33.0)), INVALID),
             ((scene_p, depth, mv, tiles, out, _params(min_velocity_pixels=nan)), INVALID),
             ((scene_p, depth, mv, tiles, out, _params(depth_extent=0.0)), INVALID),
             ((scene_p, depth, mv, tiles, out, _params(z_near=-0.1)), INVALID),
             ((scene_p, depth, mv, tiles, out, _params(jitter=(nan, 0.0))), INVALID),
             ((scene_p, depth, mv, tiles, out, _params(flags=2)), INVALID)]
    for args, status in cases:
        with pytest.raises(lib.SahError) as e:
            hip_ctx.motion_blur(*args)
        assert e.value.status == status, args
    torch.cuda.synchronize()
    assert p.out.unchanged() and p.img["tiles"].unchanged()


def test_three_frames_of_a_panning_camera_on_the_rasterised_atrium(hip_ctx):
    """frame.MotionBlur behind the rasteriser: the atrium at 128 x 72, the camera turning 6 degrees a frame with a jitter of its own each
    frame, the vectors from sah_motion_vectors_render; the output is the restatement's on the device's own planes, most of the frame blurs,
    and the sky (no surface) and the geometry both take part."""
    import torch
    w, h = 128, 72
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    view = scene.SceneView()
    view.rotate(0.0, math.radians(90.0))
    view.set_position([-7.0, 1.0, 0.0])
    view.set_render_resolution(w, h)
    view.set_perspective_projection(75.0, float(w) / float(h), 0.05)
    view.update_transforms()  # (so that the first frame has a last frame's matrices)
    blur = frame.MotionBlur(hip_ctx, 16, 16, flags=_abi.MOTION_BLUR_DITHER)  # another extent: the planes are re-created on the first frame
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    scene_bits = ref.textured_scene(w, h, 81)
    previous = None
    for n, jitter in enumerate(((0.3, -0.2), (-0.25, 0.4), (0.1, 0.1))):
        view.rotate(0.0, math.radians(6.0))
        view.jitter = np.array(jitter, f32)
        view.update_transforms()
        gb = {k: torch.zeros((h, w) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
        mv = torch.zeros((h, w, 2), dtype=torch.int16, device="cuda")
        frame.rasterised_frame(hip_ctx, geo, view.gpu_data, gb, motion_vectors=mv)
        out = blur(util.to_torch(scene_bits), gb["depth"], mv, jitter, z_near=view.near_value)
        torch.cuda.synchronize()
        got, depth_np, mv_np = util.from_torch(out, np.uint16), gb["depth"].cpu().numpy(), util.from_torch(mv, np.uint16)
        want, info = ref.motion_blur_ex(scene_bits, depth_np, mv_np, flags=ref.DITHER, z_near=view.near_value, jitter=jitter,
                                        previous_jitter=jitter if previous is None else previous)
        assert same(got, want), f"frame {n}: " + differs(got, want)
        assert same(util.from_torch(blur.tiles, np.uint16), info["tiles"])
        assert (~info["passed"]).mean() > 0.5 and (depth_np > 0).mean() > 0.5, f"frame {n}"
        previous = jitter
    assert (blur.width, blur.height, blur.render_width, blur.render_height) == (w, h, w, h)
