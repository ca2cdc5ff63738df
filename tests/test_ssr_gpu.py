"""GPU: sah_ssr (include/sah_ssr.h) against the numpy restatement of the plain march (tests/ssr_ref.py) run on the device's own planes, and its
committed fixture, bit for bit; the inputs on which a march that jumps over 8 x 8 blocks would go wrong (the kernel marches plainly today:
DESIGN.md section 5w; the cases stay for the day it does not); the identities; row windows, pitches and alignment; stream
capture and the refusals; the Python ScreenSpaceReflections over successive frames; and the frame the pass exists for — the rasterised
atrium, lit with CSM and LPV, then reflected.  The scratch plane's block is 8 x 8 texels; the trace kernel's workgroup tile is 32 x 8 pixels
(four waves of 8 x 8): the extents lie one below, at and one above both in each axis."""
import faulthandler
import os
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, mesh, scene
from tests import ssr_ref as ref
from tests import util
from tests.support import context_state, differs, Image, same, SENTINEL, side_stream_context, view_data_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_ssr as gen  # noqa: E402

f32 = np.float32
FORMATS = dict(color=_abi.FORMAT_R8G8B8A8_SRGB, normals=_abi.FORMAT_R16G16B16A16_SFLOAT, data=_abi.FORMAT_R8G8B8A8_UNORM, depth=_abi.FORMAT_D32_SFLOAT,
               source=_abi.FORMAT_R16G16B16A16_SFLOAT, lit=_abi.FORMAT_R16G16B16A16_SFLOAT, scratch=_abi.FORMAT_R32_SFLOAT, out=_abi.FORMAT_R16G16B16A16_SFLOAT)
INPUTS = ("color", "normals", "data", "depth", "source", "lit")
ORDER = INPUTS + ("scratch", "out")


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
    return _abi.SsrParams.default(**changes)


class Planes:
    """the eight device planes of one call; pitches / offsets by plane name; same_source: lit and source are one plane (the frame's lit)"""

    def __init__(self, frame_arrays, pitches=None, offsets=None, same_source=False):
        h, w = frame_arrays["depth"].shape
        self.w, self.h = w, h
        pitches, offsets = pitches or {}, offsets or {}
        self.img = {}
        for name in ORDER:
            pw, ph = ((w + 7) // 8, (h + 7) // 8) if name == "scratch" else (w, h)
            if name == "source" and same_source:
                continue
            self.img[name] = Image(FORMATS[name], pw, ph, pitches.get(name), frame_arrays[name] if name in INPUTS else None, offsets.get(name, 0))
        if same_source:
            self.img["source"] = self.img["lit"]
        self.out = self.img["out"]

    def planes(self):
        return [self.img[n].plane for n in ORDER]

    def run(self, ctx, view_data, params, rows=(0, 0)):
        import torch
        ctx.ssr(view_data, *self.planes(), params, rows)
        torch.cuda.synchronize()
        assert all(self.img[n].unchanged() for n in INPUTS), "an input changed"
        assert self.img["scratch"].unchanged(), "scratch is reserved: not written"
        return self.out.texels(np.uint16).reshape(self.h, self.w, 4)


def _check(hip_ctx, frame_arrays, view, settings, **kw):
    """one call against the restatement; -> (got, info)"""
    got = Planes(frame_arrays, **kw).run(hip_ctx, view_data_of(view), _params(**settings))
    src = frame_arrays["lit"] if kw.get("same_source") else frame_arrays["source"]
    want, info = ref.ssr_ex(**dict(frame_arrays, source=src), view=view, params=settings)
    assert same(got, want), f"{settings}: " + differs(got, want)
    return got, info


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(gen.CASES)))
def test_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture, case):
    view, params = view_data_of(gen.view()), _params(**gen.CASES[case])
    got = Planes(fixture).run(hip_ctx, view, params)
    assert same(got, fixture["out"][case]), differs(got, fixture["out"][case])
    again = Planes(fixture).run(hip_ctx, view, params)
    assert same(again, got)


# ---- extents ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    by_extent = {}
    for name, frame_arrays, view, settings in ref.parity_cases():
        by_extent.setdefault(name.split(" #")[0], []).append((frame_arrays, view, settings))
    return by_extent


@pytest.mark.parametrize("group", [f"random {w}x{h}" for w, h in ref.EXTENTS] + ["room 96x54", "room 75x41", "far 192x48"])
def test_parity_with_the_plain_march_over_extents(hip_ctx, cases, group):
    """block 8 x 8, workgroup tile 32 x 8: (7, 9), (8, 8), (9, 7) and (31, 7), (32, 8), (33, 9) lie around them; 75 and 65 are no multiple
    of 8 (a partial last block column).  Every stride, step count, refinement depth, thickness and flag of ssr_ref.RANDOM_SETTINGS."""
    assert cases[group]
    for frame_arrays, view, settings in cases[group]:
        _check(hip_ctx, frame_arrays, view, settings)


# ---- where a block skip would go wrong ---------------------------------------------------------------------------------------------------------
def _room_without_wall(w, h, keep):
    """the mirror room with its wall taken out except the texels keep(x, y) selects"""
    frame_arrays, masks = ref.mirror_room(w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    gone = masks["wall"] & ~keep(xs, ys)
    frame_arrays["depth"] = np.where(gone, f32(0), frame_arrays["depth"]).astype(f32)
    return frame_arrays, masks["wall"] & ~gone


def test_lone_texels_in_the_far_corners_of_sky_blocks(hip_ctx):
    """sky everywhere above the floor except the texel (8 bx + 7, 8 by + 7) of each block, and in a second frame (8 bx, 8 by): a block's
    nearest z is that one texel's, and the rays of the floor's columns 8 n + 7 (8 n) run into it"""
    for corner in (7, 0):
        frame_arrays, lone = _room_without_wall(96, 54, lambda xs, ys: ((xs & 7) == corner) & ((ys & 7) == corner))
        assert 20 < lone.sum() < 60
        for stride in (1.0, 2.0):
            got, info = _check(hip_ctx, frame_arrays, ref.room_view(), dict(ref.ROOM_SETTINGS, stride_pixels=stride, max_steps=256))
            on_lone = info["hit"] & lone[info["hy"], info["hx"]]
            if stride == 1.0:
                assert on_lone.sum() >= 20 and (info["outcome"] == ref.MISS_T).sum() > 500  # some rays find a lone texel; most find nothing


def test_a_block_whose_nearest_z_equals_the_rays_depth_exactly(hip_ctx):
    """the depth of one wall texel is made the ray's own zr at the sample that lands there, to the bit, and the rest of its block sky: the
    block's nearest z equals zr, dz is 0, and with thickness 0 the sample is a hit — which a skip on zr <= nearest z would jump over"""
    w, h = 96, 54
    view, settings = ref.room_view(), dict(ref.ROOM_SETTINGS, thickness=0.0, stride_pixels=2.0, refine_steps=0)
    base, masks = ref.mirror_room(w, h)
    with np.errstate(all="ignore"):
        surface, z = ref.linear_depth(base["depth"], view.z_near)
        rays = ref.Rays(ref.positions(z, view, w, h), z, ref.view_normals(base["normals"], view), view, w, h, dict(ref.DEFAULTS, **settings))
        planted = []
        frame_arrays = {k: np.array(v) for k, v in base.items()}
        for (x0, y0) in ((20, 44), (51, 40), (70, 47)):
            for i in range(1, 40):
                inside, ix, iy, zr = rays.sample(rays.t_of(i))
                tx, ty, target = int(ix[y0, x0]), int(iy[y0, x0]), zr[y0, x0]
                if not (inside[y0, x0] and masks["wall"][ty, tx]):
                    continue
                d = f32(view.z_near) / target
                near = [np.nextafter(d, f32(s), dtype=f32) for s in (0, np.inf)] + [d]
                exact = [c for c in near if f32(view.z_near) / c == target]
                if exact:
                    by, bx = ty & ~7, tx & ~7
                    frame_arrays["depth"][by:by + 8, bx:bx + 8] = 0  # the rest of the block: sky
                    frame_arrays["depth"][ty, tx] = exact[0]
                    planted.append((x0, y0, tx, ty, i))
                    break
    assert len(planted) == 3
    got, info = _check(hip_ctx, frame_arrays, view, settings)
    for x0, y0, tx, ty, i in planted:
        assert info["hit"][y0, x0] and info["hit_index"][y0, x0] == i and (info["hx"][y0, x0], info["hy"][y0, x0]) == (tx, ty)
        assert (got[y0, x0, :3] != frame_arrays["lit"][y0, x0, :3]).any()


@pytest.mark.parametrize("axis", ["y", "x"])
def test_axis_aligned_rays_with_samples_on_texel_and_block_boundaries(hip_ctx, axis):
    """The mirror room's rays run straight up their columns (ds.x is 0 but for rounding); in the room turned about the diagonal they run
    along their rows.  A ray starts at its pixel's centre, so with a stride of 1.5 or 2.5 pixels every other sample lies on an integer
    coordinate of the axis it runs along — a texel boundary, every eighth a block boundary: rows in the one room, columns in the other."""
    if axis == "y":
        frame_arrays, masks = ref.mirror_room(96, 54)
        view = ref.room_view()
    else:
        frame_arrays, masks, view = ref.transposed_room(54, 96)
    for stride in (1.5, 2.5):
        settings = dict(ref.ROOM_SETTINGS, stride_pixels=stride, max_steps=200)
        got, info = _check(hip_ctx, frame_arrays, view, settings)
        rays = info["rays"]
        floor = masks["floor"]
        along, across, start = (rays.dsy, rays.dsx, rays.s0y) if axis == "y" else (rays.dsx, rays.dsy, rays.s0x)
        assert np.abs(across[floor]).max() < 1e-2 and np.abs(along[floor]).min() > 1
        with np.errstate(all="ignore"):
            whole = [(start + rays.t_of(i) * along)[floor] for i in (1, 3, 5)]
        assert sum(int(((s == np.floor(s)) & (s > 0)).sum()) for s in whole) > 100
        assert sum(int(((s == np.floor(s)) & (s > 0) & (s % 8 == 0)).sum()) for s in whole) > 10
        assert info["hit"].mean() > 0.1


# ---- identities -------------------------------------------------------------------------------------------------------------------------------
def _facing_wall(w, h):
    """a wall facing the camera, smooth metal: every ray returns towards the near plane and finds nothing"""
    frame_arrays = ref.random_frame(w, h, 5)
    frame_arrays["depth"] = np.full((h, w), f32(0.05 / 6.0), f32)
    n = np.zeros((h, w, 4), np.float16)
    n[..., 2] = 1.0
    frame_arrays["normals"] = n.view(np.uint16)
    frame_arrays["data"][..., 1] = 10
    return frame_arrays


@pytest.mark.parametrize("only", [0, ref.REFLECTION_ONLY])
def test_identities_bit_for_bit(hip_ctx, only):
    w, h = 48, 27
    room = ref.mirror_room(w, h)[0]
    sky = dict(room, depth=np.zeros((h, w), f32))
    rough = dict(room, data=np.full((h, w, 4), 153, np.uint8))  # 153 / 255 = 0.6 in fp32: not below max_roughness
    assert ref.unorm_lut()[153] == f32(0.6)
    for name, frame_arrays, view, settings, outcomes in (("intensity 0", room, ref.room_view(), dict(ref.ROOM_SETTINGS, intensity=0.0), {ref.NO_INTENSITY, ref.ROUGH}),
                                                         ("all sky", sky, ref.room_view(), dict(ref.ROOM_SETTINGS), {ref.NO_SURFACE}),
                                                         ("all rough", rough, ref.room_view(), dict(ref.ROOM_SETTINGS), {ref.ROUGH}),
                                                         ("facing wall", _facing_wall(w, h), ref.View.of(1.0, 1.7, 0.0, 0.0, 0.05), dict(ref.DEFAULTS),
                                                          {ref.MISS_T, ref.MISS_IMAGE, ref.MISS_RAY})):
        got, info = _check(hip_ctx, frame_arrays, view, dict(settings, flags=only))
        assert set(np.unique(info["outcome"][info["surface"]])) <= outcomes | {ref.NO_SURFACE}, name
        want = np.zeros_like(got) if only else frame_arrays["lit"]
        assert same(got, want), f"{name}: " + differs(got, want)
    got, info = _check(hip_ctx, room, ref.room_view(), dict(ref.ROOM_SETTINGS, flags=only))  # (and the room itself is no identity)
    assert info["hit"].mean() > 0.1 and not same(got, np.zeros_like(got) if only else room["lit"])


def test_unclean_source_texels_spread_no_further(hip_ctx):
    w, h = 96, 54
    frame_arrays, masks = ref.mirror_room(w, h)
    clean_out, clean_info = ref.ssr_ex(view=ref.room_view(), params=ref.ROOM_SETTINGS, **frame_arrays)
    assert clean_info["hit"].mean() > 0.1
    for bits in (0x7e00, 0x7c00, 0xbc00):  # NaN, +inf, -1
        dirty = dict(frame_arrays, source=np.array(frame_arrays["source"]))
        stripe = masks["wall"] & (np.arange(h)[:, None] % 2 == 0)
        dirty["source"][stripe, 1] = bits
        got, info = _check(hip_ctx, dirty, ref.room_view(), ref.ROOM_SETTINGS)
        rejected = info["outcome"] == ref.REJECTED
        assert rejected.sum() > 100 and info["hit"].sum() > 100 and (rejected | info["hit"]).sum() == clean_info["hit"].sum()
        assert same(got[rejected], frame_arrays["lit"][rejected])
        assert np.isfinite(got.view(np.float16).astype(f32)).all()


# ---- row windows --------------------------------------------------------------------------------------------------------------------------------
def test_row_bands_write_their_rows_and_nothing_else(hip_ctx, fixture):
    W, H = gen.WIDTH, gen.HEIGHT
    view, params, whole = view_data_of(gen.view()), _params(**gen.CASES[0]), fixture["out"][0]
    assembled = np.zeros((H, W, 4), np.uint16)
    for rows in ((9, 10), (0, 7), (7, 9), (10, 18), (18, 27), (27, 27), (27, H - 1), (H - 1, H)):
        p = Planes(fixture, pitches=dict(out=W * 8 + 12))
        got = p.run(hip_ctx, view, params, rows)
        assert same(got[rows[0]:rows[1]], whole[rows[0]:rows[1]]), f"{rows}: " + differs(got[rows[0]:rows[1]], whole[rows[0]:rows[1]])
        assert p.out.padding_intact(rows), f"{rows}: out changed outside the band"
        assembled[rows[0]:rows[1]] = got[rows[0]:rows[1]]
    assert same(assembled, whole)
    assert same(Planes(fixture).run(hip_ctx, view, params, (0, H)), whole)


# ---- pitches and alignment ------------------------------------------------------------------------------------------------------------------
W_, H_ = gen.WIDTH, gen.HEIGHT
LAYOUTS = [(dict(color=W_ * 4 + 4, normals=W_ * 8 + 4, data=W_ * 4 + 12, depth=W_ * 4 + 20, source=W_ * 8 + 12, lit=W_ * 8 + 4, scratch=12 * 4 + 4, out=W_ * 8 + 20),
            dict(color=4, normals=4, data=8, depth=12, source=4, lit=12, scratch=4, out=4)),                       # nothing 8-byte aligned: dwords
           (dict(normals=W_ * 8 + 16, lit=W_ * 8 + 8, out=W_ * 8 + 24, source=W_ * 8 + 4), dict(normals=8, lit=16, out=24, source=4)),  # whole texels
           (dict(normals=W_ * 8 + 16, lit=W_ * 8 + 8, out=W_ * 8 + 24), dict(out=4)),                               # only out off: dwords
           (dict(lit=W_ * 8 + 4), dict())]                                                                        # lit's pitch off: dwords


@pytest.mark.parametrize("pitches,offsets", LAYOUTS)
@pytest.mark.parametrize("same_source", [False, True])
def test_pitches_offsets_sentinels_and_inputs(hip_ctx, fixture, pitches, offsets, same_source):
    """every plane with a pitch and an offset of its own; the 8-byte path and the dword path write the same bytes; lit as source's plane"""
    view, params = view_data_of(gen.view()), _params(**gen.CASES[0])
    frame_arrays = dict(fixture, source=fixture["lit"]) if same_source else fixture
    if same_source:
        pitches, offsets = {k: v for k, v in pitches.items() if k != "source"}, {k: v for k, v in offsets.items() if k != "source"}
    p = Planes(frame_arrays, pitches, offsets, same_source=same_source)
    got = p.run(hip_ctx, view, params)  # (asserts the inputs unchanged)
    want = ref.ssr(view=gen.view(), params=gen.CASES[0], **{k: frame_arrays[k] for k in INPUTS}) if same_source else fixture["out"][0]
    assert same(got, want), differs(got, want)
    assert p.out.padding_intact() and p.img["scratch"].padding_intact()
    assert (got != frame_arrays["lit"]).any(-1).mean() > 0.1


# ---- the call contract ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip_ctx, fixture):
    """every kind of refusal the header lists, on a context with a device and real planes: each answers its code, and afterwards `out` still
    holds its sentinel and every other plane its bytes — nothing was launched.  (tests/test_ssr_cpu.py runs the longer list of values on a
    context without a device.)"""
    import ctypes as C

    import torch
    p = Planes(fixture)
    view, ok = view_data_of(gen.view()), _params(**gen.CASES[0])
    good = dict(zip(ORDER, p.planes()))
    nan, inf = float("nan"), float("inf")

    def changed(plane, **kw):
        f = dict(ptr=plane.ptr, width=plane.width, height=plane.height, row_pitch_bytes=plane.row_pitch_bytes, format=plane.format)
        f.update(kw)
        return _abi.Plane(f["ptr"], f["width"], f["height"], f["row_pitch_bytes"], f["format"])

    def view_with(**kw):
        v = view_data_of(gen.view())
        for k, val in kw.items():
            if k == "z_near":
                v.z_near = val
            elif k.startswith("projection"):
                v.projection[int(k[10:])] = val
            else:
                v.view[int(k[4:])] = val
        return v
    INVALID, FORMAT = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
    P = lambda **kw: _params(**dict(gen.CASES[0], **kw))  # noqa: E731
    cases = []  # (what, dict(view=, planes=, params=, rows=), status)
    for n in ORDER:
        plane, bpp = good[n], _abi.FORMAT_BPP[FORMATS[n]]
        cases += [(f"{n} NULL", dict(planes=dict(good, **{n: None})), INVALID),
                  (f"{n}: null pointer", dict(planes=dict(good, **{n: changed(plane, ptr=None)})), INVALID),
                  (f"{n}: wrong format", dict(planes=dict(good, **{n: changed(plane, format=_abi.FORMAT_R32_SFLOAT if n != "scratch" else _abi.FORMAT_D32_SFLOAT)})), FORMAT),
                  (f"{n}: zero width", dict(planes=dict(good, **{n: changed(plane, width=0)})), INVALID),
                  (f"{n}: zero height", dict(planes=dict(good, **{n: changed(plane, height=0)})), INVALID),
                  (f"{n}: other width", dict(planes=dict(good, **{n: changed(plane, width=plane.width - 1)})), INVALID),
                  (f"{n}: other height", dict(planes=dict(good, **{n: changed(plane, height=plane.height - 1)})), INVALID),
                  (f"{n}: pitch shorter than a row", dict(planes=dict(good, **{n: changed(plane, row_pitch_bytes=plane.width * bpp - 4)})), INVALID),
                  (f"{n}: misaligned pointer", dict(planes=dict(good, **{n: changed(plane, ptr=plane.ptr + 2)})), INVALID),
                  (f"{n}: misaligned pitch", dict(planes=dict(good, **{n: changed(plane, row_pitch_bytes=plane.row_pitch_bytes + 2)})), INVALID)]
    cases += [("every plane of zero width", dict(planes={n: changed(good[n], width=0) for n in ORDER}), INVALID),
              ("scratch of the frame's extent", dict(planes=dict(good, scratch=changed(good["scratch"], width=W_, height=H_))), INVALID),
              ("view NULL", dict(view=None), INVALID), ("params NULL", dict(params=None), INVALID),
              ("row_end > H", dict(rows=(0, H_ + 1)), INVALID), ("row_begin > row_end", dict(rows=(9, 3)), INVALID)]
    for n in INPUTS + ("scratch",):
        cases.append((f"out is {n}'s memory", dict(planes=dict(good, out=changed(good[n], width=W_, height=H_, row_pitch_bytes=W_ * 8, format=FORMATS["out"]))), INVALID))
    for n in INPUTS:
        cases.append((f"scratch is {n}'s memory", dict(planes=dict(good, scratch=changed(good[n], width=12, height=7, row_pitch_bytes=48, format=FORMATS["scratch"]))), INVALID))
    bad = dict(max_distance=(0.0, -1.0, inf, nan), thickness=(-1.0, nan), stride_pixels=(0.5, inf, nan), max_steps=(0, 257), refine_steps=(9,),
               max_roughness=(0.0, 1.5, nan), edge_fade=(0.0, 0.6, nan), intensity=(-1.0, inf, nan), flags=(4, 0x80000000))
    for field, values in bad.items():
        cases += [(f"{field} {v}", dict(params=P(**{field: v})), INVALID) for v in values]
    for field in ("projection0", "projection5", "projection8", "projection9", "z_near", "view0", "view1", "view2", "view4", "view5", "view6", "view8", "view9", "view10"):
        cases.append((f"view: {field} NaN", dict(view=view_with(**{field: nan})), INVALID))
    cases += [(f"z_near {v}", dict(view=view_with(z_near=v)), INVALID) for v in (0.0, -0.05, inf)]
    ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
    for what, args, status in cases:
        planes, rows = args.get("planes", good), args.get("rows", (0, 0))
        got = hip_ctx.lib.sah_ssr(hip_ctx.handle, ref_of(args.get("view", view)), *[ref_of(planes[n]) for n in ORDER], ref_of(args.get("params", ok)), rows[0], rows[1])
        assert got == status, f"{what}: status {got}"
    assert len(cases) > 130
    assert hip_ctx.lib.sah_ssr(None, C.byref(view), *[C.byref(good[n]) for n in ORDER], C.byref(ok), 0, 0) == INVALID
    torch.cuda.synchronize()
    assert all(p.img[n].unchanged() for n in ORDER)  # `out` and `scratch` hold their sentinel, the inputs their bytes
    hip_ctx.ssr(view, *[good[n] for n in ORDER], ok)  # (and the well-formed call does launch)
    torch.cuda.synchronize()
    assert not p.out.unchanged()


def test_side_stream_captured_graph_replayed_and_no_side_effects(fixture):
    import torch
    with side_stream_context() as (ctx, s):
        view, params = view_data_of(gen.view()), _params(**gen.CASES[1])
        a = Planes(fixture)
        state = context_state(ctx)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.ssr(view, *a.planes(), params)
        s.synchronize()
        direct = a.out.texels(np.uint16).reshape(H_, W_, 4)
        assert same(direct, fixture["out"][1])
        assert context_state(ctx) == state
        graph = torch.cuda.CUDAGraph()  # one kernel
        with torch.cuda.graph(graph, stream=s):
            ctx.ssr(view, *a.planes(), params)
        for seed in (0, 31):  # replayed over the same inputs, then over another frame's
            if seed:
                other = gen.inputs(seed)
                b = Planes(other)
                for n in INPUTS:
                    a.img[n].t.copy_(b.img[n].t)
            else:
                other = fixture
            a.out.t.fill_(SENTINEL)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            want = ref.ssr(view=gen.view(), params=gen.CASES[1], **{k: other[k] for k in INPUTS})
            got = a.out.texels(np.uint16).reshape(H_, W_, 4)
            assert same(got, want), f"replay with seed {seed}: " + differs(got, want)
            assert (want != other["lit"]).any(-1).mean() > 0.05


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------------
def test_two_frames_through_the_python_wrapper(hip_ctx):
    """the second frame takes the first's output as its source (copied: the wrapper writes its own plane)"""
    import torch
    W, H = 96, 54
    arrays, rview, settings = ref.random_frame(W, H, 300), ref.random_view(W, H), dict(thickness=3e38, stride_pixels=2.5)
    dev = {k: util.to_torch(np.ascontiguousarray(arrays[k])) for k in INPUTS}
    ssr = frame.ScreenSpaceReflections(hip_ctx, W, H, **settings)
    assert ssr.params.refine_steps == 4 and ssr.params.max_roughness == f32(0.6) and ssr.params.flags == 0  # the header's defaults unless changed
    view = view_data_of(rview)
    first = ssr(view, dev, dev["lit"])
    torch.cuda.synchronize()
    assert first is ssr.out and tuple(ssr.scratch.shape) == (7, 12)
    want1, info = ref.ssr_ex(**dict(arrays, source=arrays["lit"]), view=rview, params=settings)
    got1 = first.cpu().numpy().view(np.uint16)
    assert same(got1, want1), differs(got1, want1)
    previous = first.clone()
    second = ssr(view, dev, dev["lit"], source=previous)
    torch.cuda.synchronize()
    want2 = ref.ssr(**dict(arrays, source=want1), view=rview, params=settings)
    got2 = second.cpu().numpy().view(np.uint16)
    assert second is ssr.out and same(got2, want2), differs(got2, want2)
    assert info["hit"].mean() > 0.1 and not same(want1, want2)  # (a reflection of last frame's reflections)
    view = view_data_of(ref.room_view())
    ssr.params = _params(**ref.ROOM_SETTINGS)
    # a frame of another extent: the wrapper re-creates its planes
    small = ref.mirror_room(48, 27)[0]
    dev = {k: util.to_torch(np.ascontiguousarray(small[k])) for k in INPUTS}
    third = ssr(view, dev, dev["lit"], source=dev["source"])
    torch.cuda.synchronize()
    want3 = ref.ssr(**small, view=ref.room_view(), params=ref.ROOM_SETTINGS)
    assert tuple(third.shape) == (27, 48, 4) and same(third.cpu().numpy().view(np.uint16), want3)


# ---- the frame the pass exists for -------------------------------------------------------------------------------------------------------------
def test_atrium_rasterised_lit_then_reflected(hip_ctx):
    """sah_gbuffer_render of the atrium at 128 x 72, sah_lighting with CSM and LPV, then sah_ssr with the header's defaults taking its
    reflections from the lit frame itself: equal to the restatement on the device's planes; the floor gains light; the sky keeps its bytes"""
    import torch
    W, H = 128, 72
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    view = scene.SceneView.default(W, H)
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    gb = {k: torch.zeros((H, W) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
    frame.rasterised_frame(hip_ctx, geo, view.gpu_data, gb)
    torch.cuda.synchronize()
    gb_np = {k: v.cpu().numpy() for k, v in gb.items()}
    gb_np["normals"] = gb_np["normals"].view(np.uint16)
    f = util.LightingFrame(W, H, gbuffer=gb_np, seed=3, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV)
    assert bytes(f.view.gpu_data) == bytes(view.gpu_data)
    lit = np.ascontiguousarray(f.run_hip(hip_ctx)).view(np.uint16).reshape(H, W, 4)
    ssr = frame.ScreenSpaceReflections(hip_ctx, W, H)
    out = ssr(view.gpu_data, gb, util.to_torch(lit))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    want, info = ref.ssr_ex(gb_np["color"], gb_np["normals"], gb_np["data"], gb_np["depth"], lit, lit, ref.View(view.gpu_data))
    assert same(got, want), differs(got, want)
    n = gb_np["normals"].view(np.float16)[..., :3].astype(f32)
    covered = gb_np["depth"] > 0
    floor = covered & (n[..., 1] < -0.9 * np.sqrt((n * n).sum(-1)))  # the world's y axis points down: the floor's normal is -y
    a, b = got.view(np.float16)[..., :3].astype(f32), lit.view(np.float16)[..., :3].astype(f32)
    brighter = (a > b).any(-1)
    print(f"atrium {W} x {H}: {float(covered.mean()):.2f} covered, {int(info['hit'].sum())} pixels reflect, {int((brighter & floor).sum())} of {int(floor.sum())} floor "
          f"pixels brighter")
    assert covered.mean() > 0.5 and floor.sum() > 50 and (brighter & floor).sum() >= 1 and not (a < b).any()
    assert same(got[~covered], lit[~covered])
