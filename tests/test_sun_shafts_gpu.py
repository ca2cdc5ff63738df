"""GPU: sah_sun_shafts (include/sah_sun_shafts.h) against the numpy restatement (tests/sun_shafts_ref.py) run on the device's own planes,
and its committed fixture, bit for bit on `out` and on `march`: extents one below, at and above the 8 x 8 wave tile and the 32 x 8
workgroup with both downscales (odd extents: the clamped footprint); D16 and D32 maps of 8 x 8 to 64 x 64 with one to four cascades, and
none; 1, 2, 31 and 64 steps with and without dither; marches that end in the first step and that never reach the surface; special depths
and lit texels; the property cases of tests/test_sun_shafts_cpu.py on the device; row windows; pitches, offsets and alignment; the
invariants; stream capture, the refusals, the argument fuzz's child process and frame.SunShafts over two frames of the rasterised atrium."""
import faulthandler
import math
import os
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, lib, mesh
from tests import layouts
from tests import sun_shafts_ref as ref
from tests import util
from tests.support import context_state, differs, Image, resized, retyped, same, SENTINEL, side_stream_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_sun_shafts as gen  # noqa: E402

f32 = np.float32
RGBA16, D32, D16 = _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_D16_UNORM
FORMATS = dict(depth=D32, lit=RGBA16, march=RGBA16, out=RGBA16)
ORDER = ("depth", "lit", "march", "out")
INPUTS = ORDER[:2]
EXTENTS = [(15, 17), (16, 16), (33, 31), (47, 49), (96, 54)]
MEDIUM = gen.MEDIUM


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)  # each test under a limit of its own: an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fixture():
    fx = np.load(gen.FIXTURE)
    return {k: fx[k] for k in fx.files}


@pytest.fixture(scope="module")
def world():
    """one view, one sun and the shadow maps the module's tests share (never written)"""
    view = ref.scene_view(96, 54)
    maps = {"d16x4": ref.noise_map(4, 64, 3, block=4), "d32x3": ref.noise_map(3, 32, 4, f32, block=2), "d16x1": ref.noise_map(1, 8, 5),
            "d32x2": ref.noise_map(2, 19, 6, f32), "d32x4": ref.noise_map(4, 8, 7, f32), "none": None}
    return dict(view=view.gpu_data, sun=ref.scene_sun(view), maps=maps)


def _params(**changes):
    return _abi.SunShaftsParams.default(**changes)


class Map:
    """a shadow map on the device, optionally with pitches of its own; bytes that belong to no texel hold SENTINEL"""

    def __init__(self, array, row_pad=0, slice_pad=0):
        import torch
        layers, h, w = array.shape
        bpp = array.dtype.itemsize
        self.row_pitch, self.slice_pitch = w * bpp + row_pad, (w * bpp + row_pad) * h + slice_pad
        host = np.full(layers * self.slice_pitch, SENTINEL, np.uint8)
        for k in range(layers):
            rows = host[k * self.slice_pitch:k * self.slice_pitch + h * self.row_pitch].reshape(h, self.row_pitch)
            rows[:, :w * bpp] = np.ascontiguousarray(array[k]).view(np.uint8).reshape(h, w * bpp)
        self.host_in = host.copy()
        self.t = torch.from_numpy(host).cuda()
        self.volume = _abi.Volume(self.t.data_ptr(), w, h, layers, self.row_pitch, self.slice_pitch, D16 if bpp == 2 else D32)

    def unchanged(self):
        return bool((self.t.cpu().numpy() == self.host_in).all())


class Planes:
    """the four device planes of one call; pitches / offsets by plane name"""

    def __init__(self, depth, lit_bits, downscale=1, pitches=None, offsets=None):
        self.h, self.w = depth.shape
        s = downscale
        pitches, offsets = pitches or {}, offsets or {}
        grid = ((self.w + s - 1) // s, (self.h + s - 1) // s)
        extent = dict(depth=(self.w, self.h), lit=(self.w, self.h), out=(self.w, self.h), march=grid)
        data = dict(depth=depth, lit=lit_bits)
        self.img = {n: Image(FORMATS[n], *extent[n], pitches.get(n), data.get(n), offsets.get(n, 0)) for n in ORDER}
        self.out = self.img["out"]

    def planes(self):
        return [self.img[n].plane for n in ORDER]

    def result(self):
        return self.out.texels(np.uint16).reshape(self.h, self.w, 4)

    def march(self):
        return self.img["march"].texels(np.uint16).reshape(self.img["march"].h, self.img["march"].w, 4)

    def run(self, ctx, world, shadow, params, rows=(0, 0)):
        import torch
        ctx.sun_shafts(world["view"], world["sun"], None if shadow is None else shadow.volume, *self.planes(), params, rows)
        torch.cuda.synchronize()
        assert all(self.img[n].unchanged() for n in INPUTS), "an input changed"
        assert shadow is None or shadow.unchanged(), "the shadow map changed"
        assert rows != (0, 0) or (self.out.padding_intact() and self.img["march"].padding_intact())  # (a windowed caller checks the other rows itself)
        return self.result()


def _same(got, want):
    return got.shape == want.shape and same(got, want)


_MAPS = {}


def _device_map(array):
    if array is None:
        return None
    if id(array) not in _MAPS:
        _MAPS[id(array)] = (array, Map(array))
    return _MAPS[id(array)][1]


def _check(hip_ctx, world, shadow, depth, lit_bits, settings, **kw):
    """one whole-frame call against the restatement, the march plane included; -> (got, info)"""
    p = Planes(depth, lit_bits, settings.get("downscale", 1), **kw)
    got = p.run(hip_ctx, world, _device_map(shadow), _params(**settings))
    want, info = ref.sun_shafts_ex(world["view"], world["sun"], shadow, depth, lit_bits, **settings)
    assert _same(p.march(), info["bits"]), f"{settings}: march " + differs(p.march(), info["bits"])
    assert _same(got, want), f"{settings}: " + differs(got, want)
    return got, info


def _frame(w, h, seed):
    return ref.box_depth(w, h, seed=seed), ref.textured_lit(w, h, seed)


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(gen.CASES)))
def test_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture, case):
    name, settings = gen.CASES[case]
    view, sun = gen.structures(fixture)
    w = dict(view=view, sun=sun)
    p = Planes(fixture["depth"], fixture["lit"], settings.get("downscale", 1))
    shadow = _device_map(gen.shadow_map(fixture, name))
    got = p.run(hip_ctx, w, shadow, _params(**settings))
    assert _same(p.march(), fixture[f"march{case}"]), "march " + differs(p.march(), fixture[f"march{case}"])
    assert _same(got, fixture["out"][case]), differs(got, fixture["out"][case])
    again = p.run(hip_ctx, w, shadow, _params(**settings))  # two calls, the same bytes
    assert _same(again, got)


# ---- extents, maps and parameters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("downscale", [1, 2])
@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: f"{e[0]}x{e[1]}")
def test_parity_over_extents_maps_step_counts_and_dither(hip_ctx, world, extent, downscale):
    w, h = extent
    depth, lit = _frame(w, h, 100 + w)
    taps = 0
    for name, settings in (("d16x4", dict(num_steps=31, flags=ref.DITHER)), ("d32x3", dict(num_steps=64, step_length=0.3)), ("d16x1", dict(num_steps=2, step_length=4.0)),
                           ("d32x2", dict(num_steps=1, step_length=3.0, flags=ref.DITHER, dither_offset=9)), ("d32x4", dict()), ("none", dict(num_steps=31))):
        _, info = _check(hip_ctx, world, world["maps"][name], depth, lit, dict(MEDIUM, downscale=downscale, **settings))
        taps += info["taps"]
        assert info["samples"]
    assert taps


def test_marches_that_end_in_the_first_step_and_that_never_reach_the_surface(hip_ctx, world):
    w, h = 47, 49
    depth, lit = ref.box_depth(w, h, holes=False), ref.textured_lit(w, h, 7)  # (no sky: its rays run the full march)
    for downscale in (1, 2):
        _, info = _check(hip_ctx, world, world["maps"]["d16x4"], depth, lit, dict(MEDIUM, downscale=downscale, step_length=100.0, num_steps=4))
        assert (info["L"] < 100.0).all() and info["samples"] == info["L"].size  # every ray ends inside step 0
        _, info = _check(hip_ctx, world, world["maps"]["d16x4"], depth, lit, dict(MEDIUM, downscale=downscale, step_length=0.001, num_steps=2, flags=ref.DITHER))
        assert (depth < info["d_min"]).all() and info["samples"] == 2 * info["L"].size  # every surface lies beyond the march: two full steps per ray


def test_special_depths_and_lit_texels(hip_ctx, world):
    w, h = 33, 31
    depth, lit = _frame(w, h, 8)
    depth = depth.copy()
    depth[::3, ::2], depth[1::3, 1::2], depth[2::5, ::3], depth[::7, 1::3], depth[4, 4] = 0.0, np.nan, 1e-40, -1.0, np.inf
    lit = lit.copy()
    for (x, y, c, bits) in ((20, 12, 0, 0x7E00), (21, 30, 1, 0x7C00), (3, 17, 2, 0xBC00), (30, 25, 0, 0xFC00), (9, 9, 3, 0x7E00)):
        lit[y, x, c] = bits
    for downscale in (1, 2):
        got, _ = _check(hip_ctx, world, world["maps"]["d32x3"], depth, lit, dict(MEDIUM, downscale=downscale))
        assert (got[12, 20] == lit[12, 20]).all() and (got[30, 21] == lit[30, 21]).all() and (got[25, 30] == lit[25, 30]).all()  # not finite: lit's bits
        assert (got[17, 3] != lit[17, 3]).any() and got[9, 9, 3] == 0x7E00  # a negative texel is arithmetic like any other; alpha is never read


# ---- the property cases of the CPU test, on the device -----------------------------------------------------------------------------------
def test_a_step_transmittance_of_one_is_the_identity_on_the_device(hip_ctx, world):
    w, h = 47, 49
    depth, lit = _frame(w, h, 9)
    for downscale in (1, 2):
        got, info = _check(hip_ctx, world, world["maps"]["d16x4"], depth, lit, dict(MEDIUM, downscale=downscale, step_transmittance=1.0, flags=ref.DITHER))
        assert _same(got, lit) and (info["bits"] == np.array([0, 0, 0, 0x3C00], np.uint16)).all()


def test_an_occluded_map_leaves_the_ambient_term_on_the_device(hip_ctx, world):
    w, h = 33, 31
    depth, lit = _frame(w, h, 10)
    dark = ref.constant_map(4, 16, 0, np.uint16)  # every compare fails: nothing is lit
    _, info = _check(hip_ctx, world, dark, depth, lit, dict(MEDIUM, flags=ref.TERM_ONLY))
    assert info["taps"] > 0
    full = info["V"] == 0
    assert full.any() and (info["S"][full] == (info["E"][full, None] * np.array(MEDIUM["ambient"], f32))).all()


def test_sky_and_a_surface_at_the_clip_distance_agree_on_the_device(hip_ctx, world):
    w, h = 16, 16
    lit = ref.textured_lit(w, h, 11)
    settings = dict(MEDIUM, num_steps=16)
    d_min = f32(world["view"].z_near) / (f32(0.5) * f32(16))
    sky, _ = _check(hip_ctx, world, world["maps"]["d16x4"], np.zeros((h, w), f32), lit, settings)
    wall, _ = _check(hip_ctx, world, world["maps"]["d16x4"], np.full((h, w), d_min, f32), lit, settings)
    assert _same(sky, wall) and not _same(sky, lit)


def test_no_map_a_walls_shadow_and_a_depth_step_on_the_device(hip_ctx, world):
    """properties (b), (c), (e) and (g) of tests/test_sun_shafts_cpu.py with the device's planes held to the restatement's"""
    w, h = 48, 40
    lit = ref.textured_lit(w, h, 12)
    flat = np.full((h, w), 0.008, f32)
    _, info = _check(hip_ctx, world, None, flat, lit, dict(MEDIUM, anisotropy=0.0, num_steps=16, step_length=0.75, step_transmittance=0.9))
    assert (info["V"] == info["E"]).all() and (info["ph"] == ref.INV_4PI).all() and ((info["T"] > 0) & (info["T"] < 1)).all()
    wall = np.ones((4, 64, 64), f32)
    wall[:, :32, :] = 0.0
    depth = ref.box_depth(w, h, holes=False)
    for downscale in (1, 2):
        _, info = _check(hip_ctx, world, wall, depth, lit, dict(MEDIUM, downscale=downscale))
        assert (info["V"] == info["E"]).mean() >= 0.25 and (info["V"] < info["E"]).mean() >= 0.25
    stepped = np.full((h, w), f32(world["view"].z_near), f32)
    stepped[:h // 2, :w // 2] = f32(world["view"].z_near) / f32(100.0)
    for sharpness in (50.0, 0.0):
        _check(hip_ctx, world, world["maps"]["d16x4"], stepped, lit, dict(MEDIUM, downscale=2, depth_sharpness=sharpness, flags=ref.DITHER, num_steps=64))


# ---- row windows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("downscale", [1, 2])
def test_row_windows_cover_the_frame_and_write_nothing_else(hip_ctx, world, downscale):
    import torch
    w, h = 47, 49
    depth, lit = _frame(w, h, 41)
    settings = dict(MEDIUM, downscale=downscale, flags=ref.DITHER)
    shadow = _device_map(world["maps"]["d16x4"])
    want, info = ref.sun_shafts_ex(world["view"], world["sun"], world["maps"]["d16x4"], depth, lit, **settings)
    whole = Planes(depth, lit, downscale).run(hip_ctx, world, shadow, _params(**settings))
    assert _same(whole, want)
    banded = Planes(depth, lit, downscale)
    for rows in ((0, 7), (7, 8), (8, 24), (24, 24), (24, 41), (41, h)):  # windows that split the 8-row groups; a one-row and an empty window
        before = banded.result().copy()
        single = Planes(depth, lit, downscale)
        got = single.run(hip_ctx, world, shadow, _params(**settings), rows)
        assert _same(got[rows[0]:rows[1]], want[rows[0]:rows[1]]), f"rows {rows}: " + differs(got[rows[0]:rows[1]], want[rows[0]:rows[1]])
        layouts.assert_rows_untouched(np.uint16(SENTINEL * 0x101), got, rows[0], rows[1], what=f"rows {rows}")
        m0, m1 = (rows if downscale == 1 else (rows[0] // 2, min((rows[1] - 1) // 2 + 2, (h + 1) // 2))) if rows[1] > rows[0] else (0, 0)
        assert _same(single.march()[m0:m1], info["bits"][m0:m1])
        layouts.assert_rows_untouched(np.uint16(SENTINEL * 0x101), single.march(), m0, m1, what=f"march rows of {rows}")
        banded.run(hip_ctx, world, shadow, _params(**settings), rows)
        layouts.assert_rows_untouched(before, banded.result(), rows[0], rows[1], what=f"rows {rows} of the union")
    torch.cuda.synchronize()
    assert _same(banded.result(), whole) and _same(banded.march(), info["bits"])


# ---- layout -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("downscale", [1, 2])
def test_pitched_offset_and_misaligned_planes_give_the_same_bytes(hip_ctx, world, downscale):
    w, h = 47, 49
    depth, lit = _frame(w, h, 51)
    settings = dict(MEDIUM, downscale=downscale, flags=ref.DITHER)
    tight, _ = _check(hip_ctx, world, world["maps"]["d16x4"], depth, lit, settings)  # torch allocations: 256-byte aligned
    mw = (w + downscale - 1) // downscale
    for kw in (dict(offsets=dict(lit=4)), dict(offsets=dict(out=4)), dict(offsets=dict(march=4, depth=12)),
               dict(pitches=dict(lit=w * 8 + 16, out=w * 8 + 32, depth=w * 4 + 12, march=mw * 8 + 8)),
               dict(pitches=dict(lit=w * 8 + 4, out=w * 8 + 12, march=mw * 8 + 4), offsets=dict(lit=16, out=16))):
        got, _ = _check(hip_ctx, world, world["maps"]["d16x4"], depth, lit, settings, **kw)
        assert _same(got, tight), kw


def test_a_pitched_shadow_map_gives_the_same_bytes(hip_ctx, world):
    w, h = 33, 31
    depth, lit = _frame(w, h, 52)
    for name, pads in (("d16x4", (6, 10)), ("d32x3", (12, 64))):
        settings = dict(MEDIUM, flags=ref.DITHER)
        want, _ = _check(hip_ctx, world, world["maps"][name], depth, lit, settings)
        p = Planes(depth, lit)
        got = p.run(hip_ctx, world, Map(world["maps"][name], *pads), _params(**settings))
        assert _same(got, want), name


@pytest.mark.parametrize("spec", [dict(row_pad=8, offset=8), dict(row_pad=40, offset=16)], ids=["A", "B"])
def test_layouts_of_tests_layouts(hip_ctx, world, spec):
    """the two families of tests/layouts.py: the smallest padding and offset the argument check admits, and a padding that is a multiple of
    the texel but not of 16 — same bytes as the tight run, no padding byte written, inputs unchanged"""
    import torch
    w, h = 33, 31
    depth, lit = _frame(w, h, 61)
    settings = dict(MEDIUM, downscale=2)
    want, info = ref.sun_shafts_ex(world["view"], world["sun"], world["maps"]["d16x4"], depth, lit, **settings)
    arrays = dict(depth=torch.from_numpy(depth).cuda(), lit=util.to_torch(lit), march=torch.full((16, 17, 4), 0x5A5A, dtype=torch.int16, device="cuda"),
                  out=torch.full((h, w, 4), 0x5A5A, dtype=torch.int16, device="cuda"))
    small = dict(row_pad=spec["row_pad"] // 2, offset=spec["offset"] // 2)  # the 4-byte texels
    wrapped = layouts.wrap(arrays, {n: (FORMATS[n], 2) for n in ORDER}, dict(lit=spec, out=spec, march=spec, depth=small))
    hip_ctx.sun_shafts(world["view"], world["sun"], _device_map(world["maps"]["d16x4"]).volume, *[wrapped[n].plane() for n in ORDER], _params(**settings))
    torch.cuda.synchronize()
    assert _same(wrapped["out"].read(np.uint16), want) and _same(wrapped["march"].read(np.uint16), info["bits"])
    layouts.assert_padding_intact(wrapped, what=str(spec))
    layouts.assert_inputs_unchanged({n: wrapped[n] for n in INPUTS}, what=str(spec))


# ---- runtime ------------------------------------------------------------------------------------------------------------------------------
def test_side_stream_under_capture_and_replayed_over_other_inputs(fixture):
    import torch
    fx = fixture
    name, settings = gen.CASES[1]
    view, sun = gen.structures(fx)
    shadow = _device_map(gen.shadow_map(fx, name))
    with side_stream_context() as (ctx, s):
        a = Planes(fx["depth"], fx["lit"], settings["downscale"])
        params = _params(**settings)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.sun_shafts(view, sun, shadow.volume, *a.planes(), params)
        s.synchronize()
        assert _same(a.result(), fx["out"][1])
        depth_b, lit_b = _frame(gen.WIDTH, gen.HEIGHT, 71)
        b = Planes(depth_b, lit_b, settings["downscale"])
        direct = ref.sun_shafts(view, sun, gen.shadow_map(fx, name), depth_b, lit_b, **settings)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.sun_shafts(view, sun, shadow.volume, *a.planes(), params)
        for n in INPUTS:
            a.img[n].t.copy_(b.img[n].t)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(a.result(), direct) and not _same(direct, fx["out"][1])


def test_no_side_effects_on_the_context(hip_ctx, fixture):
    f = util.LightingFrame(64, 36, seed=5, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flavour="atrium")
    f.run_hip(hip_ctx)

    def state():
        return context_state(hip_ctx)
    before = state()
    view, sun = gen.structures(fixture)
    got = Planes(fixture["depth"], fixture["lit"]).run(hip_ctx, dict(view=view, sun=sun), _device_map(fixture["map_d16"]), _params(**gen.CASES[0][1]))
    assert state() == before and _same(got, fixture["out"][0])


def test_every_refusal_of_the_header_on_the_device(hip_ctx):
    """Every refused entry of tests/test_sun_shafts_cpu.py's list — each refusal the header names, the 2^32 texels among them — on a context
    with a device, its planes and its map rebuilt inside one device allocation: the status is the header's, and since nothing is launched
    not one byte of the allocation changes.  (The list's well-formed calls are the other tests of this file.)"""
    import torch
    from tests.test_sun_shafts_cpu import OK, _cases, _invoke
    slots = 24  # the list puts its planes at base + (0..3) * 64 KiB and its map at base + 8 * 64 KiB; two slots of margin in front
    memory = torch.full((slots << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    base = memory.data_ptr() + (2 << 16)
    assert base % 256 == 0
    torch.cuda.synchronize()
    refused = 0
    for name, args, want in _cases(base):
        if want == OK:
            continue
        got = _invoke(hip_ctx.lib, hip_ctx.handle, args)
        assert got == want, f"{name}: status {got}"
        refused += 1
    torch.cuda.synchronize()
    assert refused > 100 and bool((memory == SENTINEL).all())
    out, info = None, None  # (the context still works)
    depth, lit = _frame(16, 16, 3)
    view = ref.scene_view(16, 16)
    out, info = _check(hip_ctx, dict(view=view.gpu_data, sun=ref.scene_sun(view)), None, depth, lit, dict(MEDIUM))
    assert info["samples"]


def test_the_dither_offset_permutes_the_sixteen_offsets_on_the_device(hip_ctx, world):
    """property (h) on a 4 x 4 march: with dither_offset running 0..15 every texel of the device's march plane is the restatement's for the
    offset (b + dither_offset) & 15 of its matrix entry b, so each texel meets all sixteen offsets; the sixteen planes are not all equal"""
    w, h = 4, 4
    depth, lit = np.full((h, w), 0.004, f32), ref.textured_lit(w, h, 13)
    my, mx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    planes, seen = [], []
    for offset in range(16):
        settings = dict(MEDIUM, flags=ref.DITHER | ref.TERM_ONLY, dither_offset=offset, num_steps=8, step_length=2.0)
        got, info = _check(hip_ctx, world, world["maps"]["d16x4"], depth, lit, settings)
        planes.append(got)
        seen.append(ref.dither(mx, my, offset, ref.DITHER))
    levels = ((np.arange(16, dtype=f32) + f32(0.5)) * f32(0.0625)).tolist()
    assert all(sorted(np.stack(seen)[:, j, i].tolist()) == levels for j in range(h) for i in range(w))
    assert len({p.tobytes() for p in planes}) > 8  # the offset reaches the device's samples


def test_transmittance_falls_with_depth_on_the_device(hip_ctx, world):
    """property (c): constant-depth frames ever farther away; the device's stored T lies in [0, 1] and never rises, pixel by pixel"""
    w, h = 33, 31
    lit = ref.textured_lit(w, h, 14)
    last = None
    for distance in (0.3, 1.0, 3.0, 9.0, 40.0):
        depth = np.full((h, w), f32(world["view"].z_near) / f32(distance), f32)
        p = Planes(depth, lit)
        p.run(hip_ctx, world, _device_map(world["maps"]["d16x4"]), _params(**MEDIUM))
        info = ref.march(world["view"], world["sun"], world["maps"]["d16x4"], depth, **MEDIUM)
        assert _same(p.march(), info["bits"])
        T = ref.h2f(p.march()[..., 3])
        assert ((T >= 0) & (T <= 1)).all()
        if last is not None:
            assert (T <= last).all() and (T < last).any()
        last = T
    assert (last < 0.6).all()


def test_refusals_launch_nothing(hip_ctx, world, fixture):
    """a hand-picked list on the planes of a real call (test_every_refusal_of_the_header_on_the_device runs the whole list): the targets keep
    their bytes"""
    import torch
    p = Planes(fixture["depth"], fixture["lit"])
    depth, lit, march, out = p.planes()
    view, sun = world["view"], world["sun"]
    shadow = _device_map(world["maps"]["d16x4"]).volume
    ok = _params()

    def relayered(volume, layers):
        return _abi.Volume(volume.ptr, volume.width, volume.height, layers, volume.row_pitch_bytes, volume.slice_pitch_bytes, volume.format)
    INVALID, FORMAT = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
    nan = float("nan")
    cases = [((view, sun, shadow, depth, lit, march, retyped(out, _abi.FORMAT_R32_SFLOAT), ok), FORMAT),
             ((view, sun, shadow, retyped(depth, _abi.FORMAT_R32_SFLOAT), lit, march, out, ok), FORMAT),
             ((view, sun, shadow, depth, lit, retyped(march, _abi.FORMAT_R16G16_SFLOAT), out, ok), FORMAT),
             ((view, sun, retyped(shadow, RGBA16), depth, lit, march, out, ok), FORMAT),
             ((view, sun, relayered(shadow, 0), depth, lit, march, out, ok), INVALID),
             ((None, sun, shadow, depth, lit, march, out, ok), INVALID),
             ((view, None, shadow, depth, lit, march, out, ok), INVALID),
             ((view, sun, shadow, depth, None, march, out, ok), INVALID),
             ((view, sun, shadow, depth, lit, march, out, None), INVALID),
             ((view, sun, shadow, depth, lit, march, out, ok, (0, gen.HEIGHT + 1)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, ok, (9, 3)), INVALID),
             ((view, sun, shadow, depth, lit, resized(march, 48, 27), out, ok), INVALID),       # the grid of downscale 2 under downscale 1
             ((view, sun, shadow, depth, lit, march, out, _params(downscale=2)), INVALID),      # and the reverse
             ((view, sun, shadow, resized(depth, 95, 54), lit, march, out, ok), INVALID),
             ((view, sun, shadow, depth, lit, march, lit, ok), INVALID),                        # in place
             ((view, sun, shadow, depth, lit, lit, out, ok), INVALID),                          # march over an input
             ((view, sun, shadow, depth, lit, march, out, _params(num_steps=0)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(num_steps=65)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(step_length=0.0)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(step_transmittance=0.0)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(step_transmittance=1.5)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(anisotropy=1.0)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(albedo=(1.0, nan, 1.0))), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(depth_sharpness=-1.0)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(downscale=3)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(dither_offset=16)), INVALID),
             ((view, sun, shadow, depth, lit, march, out, _params(flags=4)), INVALID)]
    for args, status in cases:
        with pytest.raises(lib.SahError) as e:
            hip_ctx.sun_shafts(*args)
        assert e.value.status == status, args
    torch.cuda.synchronize()
    assert p.out.unchanged() and p.img["march"].unchanged()


def test_the_argument_fuzz_never_reaches_a_device():
    """tests/sun_shafts_fuzz_child.py in a fresh child process.  Its made-up addresses must not reach a GPU, so it throws its descriptors
    at a context without a device; where a device is present (this test's machines) it has to say so and make no call — the 2000
    iterations themselves run where there is none, from tests/test_sun_shafts_cpu.py."""
    import re
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sun_shafts_fuzz_child.py"), "53", "200"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=100)
    assert r.returncode == 0, r.stdout[-2000:]
    assert ("SKIP: a HIP device is present" in r.stdout) != ("OK: 200 iterations" in r.stdout), r.stdout[-2000:]
    assert not re.search(r"\bok: \d", r.stdout)  # no call of the fuzz was ever launched


def test_two_frames_of_the_rasterised_atrium(hip_ctx):
    """frame.SunShafts behind the rasteriser: the atrium at 128 x 72 with the cascades fitted to the camera and a blocky map, the camera
    turning between the frames, through rasterised_frame's opt-in; the output is the restatement's on the device's own depth with the
    extinction turned into a step transmittance by the helper and the dither offset stepping per frame."""
    import torch
    w, h = 128, 72
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    view = ref.scene_view(w, h)
    sun = ref.scene_sun(view)
    shadow = ref.noise_map(4, 64, 21, block=8)
    shadow_t = util.to_torch(shadow)
    shafts = frame.SunShafts(hip_ctx, 16, 16, extinction=0.05, flags=_abi.SUN_SHAFTS_DITHER, downscale=2, ambient=(2e-6, 3e-6, 5e-6))  # another extent: re-created
    assert shafts.params.step_transmittance == f32(math.exp(-0.05 * 0.5))
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    lit = ref.textured_lit(w, h, 81)
    for n in range(2):
        view.rotate(0.0, math.radians(6.0))
        view.update_transforms()
        gb = {k: torch.zeros((h, w) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
        opt = dict(sun=sun, shadowmap=shadow_t, lit=util.to_torch(lit))
        opt["pass"] = shafts
        frame.rasterised_frame(hip_ctx, geo, view.gpu_data, gb, sun_shafts=opt)
        torch.cuda.synchronize()
        got, depth_np = util.from_torch(opt["out"], np.uint16), gb["depth"].cpu().numpy()
        want, info = ref.sun_shafts_ex(view.gpu_data, sun, shadow, depth_np, lit, downscale=2, flags=ref.DITHER, dither_offset=n, ambient=(2e-6, 3e-6, 5e-6),
                                       albedo=(_abi.LIGHTING_EXPOSURE,) * 3, step_transmittance=float(shafts.params.step_transmittance))
        assert _same(got, want), f"frame {n}: " + differs(got, want)
        assert _same(util.from_torch(shafts.march, np.uint16), info["bits"])
        assert (got != lit).any(-1).mean() > 0.9 and 0.05 < (depth_np > 0).mean() and info["taps"] > 0, f"frame {n}"
    assert (shafts.width, shafts.height) == (w, h)
