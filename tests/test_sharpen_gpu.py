"""GPU: sah_sharpen (include/sah_sharpen.h) against the numpy restatement (tests/sharpen_ref.py) run on the device's own planes, and the
committed fixture.  Every comparison is bit for bit over every pixel; every output plane is pre-filled with a pattern and surrounded by
guard bytes, and every check looks at them.  The kernel's tile is 64 x 16 pixels, four adjacent pixels of a row per thread; the main input
is the blocky image tests/test_sharpen_cpu.py shows to be sharpened almost everywhere."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, lib
from tests import layouts
from tests import sharpen_ref as ref
from tests import util
from tests.host_programs import host_program
from tests.support import context_state, differs, hip_runtime, Image, retyped, SENTINEL, side_stream_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_sharpen as gen  # noqa: E402

f32 = np.float32
RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT
TW, TH = ref.TILE
PATTERN = 0x0101 * SENTINEL  # what every half of an untouched output plane holds


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)  # each test under a limit of its own: an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fixture():
    fx = np.load(gen.FIXTURE)
    return {"scene": np.ascontiguousarray(fx["scene_plane"][:, :gen.WIDTH]), "sharpened": fx["sharpened"]}


class State:
    """a 16-byte device exposure state inside a larger allocation of sentinel bytes; `exposure` None = no state (NULL)"""

    def __init__(self, exposure, offset=16):
        import torch
        host = np.full(64, SENTINEL, np.uint8)
        self.offset = offset
        if exposure is not None:
            host[offset:offset + 16] = np.frombuffer(np.array([exposure, -1.5, 0, 0], f32).tobytes(), np.uint8)
        self.host_in = host.copy()
        self.t = torch.from_numpy(host).cuda()
        self.ptr = None if exposure is None else self.t.data_ptr() + offset

    def unchanged(self):
        return bool((self.t.cpu().numpy() == self.host_in).all())


def _texels(img):
    return img.texels(np.uint16).reshape(img.h, img.w, 4)


def _check(ctx, scene_np, settings=None, exposure=None, pitches=(None, None), offsets=(0, 0), rows=(0, 0)):
    """one call against the restatement: the rows of the band, the rows outside it, the guard bytes, the inputs; returns the texels of out"""
    import torch
    h, w = scene_np.shape[:2]
    scene_img = Image(RGBA16F, w, h, pitches[0], scene_np, offsets[0])
    out_img = Image(RGBA16F, w, h, pitches[1], None, offsets[1])
    state = State(exposure)
    ctx.sharpen(scene_img.plane, state.ptr, out_img.plane, _abi.SharpenParams.default(**(settings or {})), rows)
    torch.cuda.synchronize()
    got = _texels(out_img)
    want = ref.sharpen(scene_np, exposure, settings, rows, out=np.full(scene_np.shape, PATTERN, np.uint16))
    assert got.tobytes() == want.tobytes(), f"{w} x {h}, {settings}, exposure {exposure}, rows {rows}: " + differs(got, want)
    assert out_img.padding_intact(ref_rows(rows, h)), "bytes outside the band's texels changed"
    assert scene_img.unchanged() and state.unchanged()
    return got


def ref_rows(rows, h):
    return (0, h) if tuple(rows) == (0, 0) else tuple(rows)


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
def test_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture):
    for (exposure, settings), want in zip(gen.CASES, fixture["sharpened"]):
        got = _check(hip_ctx, fixture["scene"], settings, exposure)
        assert got.tobytes() == want.tobytes(), f"{settings}, exposure {exposure}: " + differs(got, want)
        assert _check(hip_ctx, fixture["scene"], settings, exposure).tobytes() == got.tobytes()


# ---- extents ------------------------------------------------------------------------------------------------------------------------------
# tile 64 x 16: single pixels and lines, one below, at and one above the tile in both dimensions, two tiles and one more
@pytest.mark.parametrize("extent", [(1, 1), (1, 7), (5, 1), (3, 3), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW + 1, 2 * TH + 1)])
def test_extents(hip_ctx, extent):
    w, h = extent
    assert extent in [(1, 1), (1, 7), (5, 1), (3, 3), (63, 15), (64, 16), (65, 17), (129, 33)]
    scene_np = ref.blocky_inputs(w, h, 11 * w + h, unclean=3 if w * h >= 64 else 0)
    for flags in (0, ref.DENOISE):
        got = _check(hip_ctx, scene_np, dict(flags=flags))
        if w * h >= 64:
            assert (got[..., :3] != scene_np[..., :3]).any(-1).mean() > 0.8  # not a comparison of pass-through


# ---- both paths ---------------------------------------------------------------------------------------------------------------------------
# pitches and offsets in bytes: scene, out; width 69 (tight rows: 552 bytes)
@pytest.mark.parametrize("pitches,offsets", [((560, 576), (0, 16)),                  # padded, 16-byte aligned: the 16-byte path
                                             ((69 * 8 + 4, 69 * 8 + 12), (4, 8)),    # no plane 16-byte aligned: dwords
                                             ((560, 576), (0, 8)),                   # out 8-byte aligned only: dwords
                                             ((560, 568), (0, 0)),                   # one pitch off the 16 bytes: dwords
                                             ((552, 552), (0, 0)),                   # tight rows of an odd width: dwords
                                             ((556, 560), (12, 0))])                 # the scene off, out aligned: dwords
def test_pitches_and_offsets(hip_ctx, fixture, pitches, offsets):
    for (exposure, settings), want in zip(gen.CASES[1:3], fixture["sharpened"][1:3]):
        got = _check(hip_ctx, fixture["scene"], settings, exposure, pitches, offsets)
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("spec", [dict(row_pad=8, offset=8), dict(row_pad=40, offset=24), dict(row_pad=8, offset=32)])
def test_layout_helpers_padded_planes_equal_the_tight_run(hip_ctx, spec):
    """tests/layouts.py: the same logical image tight (552-byte rows: dwords) and padded — a 16-byte pitch off a 16-byte base and a base
    that is a multiple of the texel only (dwords both), then a 16-byte pitch on a 16-byte base (the 16-byte path) — with NaN bytes in the
    scene's padding, so that a padding read which reaches a result poisons it"""
    import torch
    w, h = TW + 5, TH + 3
    scene_np = ref.blocky_inputs(w, h, 31, unclean=4)
    want = ref.sharpen(scene_np, None, dict(flags=ref.DENOISE))
    results = []
    for layout in (None, spec):
        scene_p = layouts.pitched(util.to_torch(scene_np), RGBA16F, 2, layout, fill=layouts.NAN_FILL)
        out_p = layouts.pitched(torch.full((h, w, 4), 0x1234, dtype=torch.int16, device="cuda"), RGBA16F, 2, layout)
        hip_ctx.sharpen(scene_p.plane(), None, out_p.plane(), _abi.SharpenParams.default(flags=_abi.SHARPEN_DENOISE))
        torch.cuda.synchronize()
        layouts.assert_padding_intact(scene_p, out_p, what=f"sharpen {layout}")
        layouts.assert_inputs_unchanged(scene_p, what=f"sharpen {layout}")
        results.append(out_p.read(np.uint16))
    assert results[1].tobytes() == want.tobytes(), differs(results[1], want)
    assert results[0].tobytes() == results[1].tobytes()


# ---- flags and parameters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, ref.DENOISE])
def test_flags_and_parameters(hip_ctx, flags):
    scene_np = ref.blocky_inputs(TW + 3, TH + 2, 77, unclean=2)
    seen = set()
    for sharpness in (0.0, 0.5, 1.0):
        for pre_scale in (1.0, 0.25):
            got = _check(hip_ctx, scene_np, dict(sharpness=sharpness, pre_scale=pre_scale, flags=flags))
            seen.add(got.tobytes())
    assert len(seen) >= 5  # (sharpness 0 may give one picture under both scales)
    # sharpness 0 with k = 1: the scene itself, bit for bit (values far below 4096; the planted -0 comes out as +0)
    got = _check(hip_ctx, scene_np, dict(sharpness=0.0, flags=flags))
    same = (got == scene_np).all(-1)
    assert same.mean() > 0.99 and ((scene_np[~same][:, :3] == 0x8000).any(-1)).all()


def test_image_scales_from_a_thousandth_to_the_largest_half(hip_ctx):
    g = np.random.default_rng(9)
    for maximum in (1e-3, 64.0, 65504.0):
        img = g.uniform(0, 1, (TH + 1, TW + 1, 4)) ** 3 * maximum
        img[g.random(img.shape[:2]) < 0.1, :3] = 0
        scene_np = np.minimum(img, 65504.0).astype(np.float16).view(np.uint16)
        got = _check(hip_ctx, scene_np, dict(flags=ref.DENOISE))
        halfs = got.view(np.float16)[..., :3]
        assert np.isfinite(halfs).all() and (halfs >= 0).all()


# ---- the device exposure state ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exposure,k", [(None, 0.25), (0.375, 0.25 * 0.375), (float("nan"), 0.25), (0.0, 0.25), (2.0 ** 23, 0.25),
                                        (float("inf"), 0.25), (-2.0, 0.25), (2.0 ** -19, 0.25), (2.0 ** 22, 2.0 ** 20), (2.0 ** -18, 2.0 ** -20)])
def test_the_device_exposure_state(hip_ctx, exposure, k):
    assert ref.scale_of(0.25, exposure) == f32(k)  # the expected k: pre_scale, or pre_scale * exposure within [2^-20, 2^20]
    scene_np = ref.blocky_inputs(TW + 1, TH + 1, 5, unclean=2)
    got = _check(hip_ctx, scene_np, dict(pre_scale=0.25, flags=ref.DENOISE), exposure)
    # what the fallback means: the bytes of the call without a state
    if k == 0.25:
        assert got.tobytes() == ref.sharpen(scene_np, None, dict(pre_scale=0.25, flags=ref.DENOISE), out=np.full(scene_np.shape, PATTERN, np.uint16)).tobytes()


# ---- row bands ----------------------------------------------------------------------------------------------------------------------------------
def test_row_bands_at_and_around_a_tile_boundary(hip_ctx):
    w, h = TW + 6, 2 * TH + 1
    scene_np = ref.blocky_inputs(w, h, 19, unclean=5)
    scene_np[TH - 1, 7, 0] = scene_np[TH, 40, 1] = 0x7e00  # unclean texels on both sides of the tile's row boundary
    settings = dict(flags=ref.DENOISE)
    full = _check(hip_ctx, scene_np, settings, 0.5)
    for rows in ((0, TH - 1), (0, TH), (0, TH + 1), (TH - 1, TH), (TH, TH + 1), (TH - 1, h), (TH, h), (TH + 1, h), (1, 2), (h - 1, h), (5, 5), (h, h)):
        got = _check(hip_ctx, scene_np, settings, 0.5, rows=rows)  # (compares the band, and everything outside it with what out held before)
        assert got[rows[0]:rows[1]].tobytes() == full[rows[0]:rows[1]].tobytes(), rows
        layouts.assert_rows_untouched(np.uint16(PATTERN), got, rows[0], rows[1], what=f"rows {rows}")
    # two adjacent bands into one plane, on a pitched plane: the full frame
    for split in (TH - 1, TH, TH + 1):
        import torch
        scene_img, out_img = Image(RGBA16F, w, h, w * 8 + 4, scene_np, 4), Image(RGBA16F, w, h, w * 8 + 12, None, 8)
        state = State(0.5)
        for rows in ((0, split), (split, h)):
            hip_ctx.sharpen(scene_img.plane, state.ptr, out_img.plane, _abi.SharpenParams.default(**settings), rows)
        torch.cuda.synchronize()
        assert _texels(out_img).tobytes() == full.tobytes() and out_img.padding_intact() and scene_img.unchanged()


# ---- unclean texels -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0x7e00, 0x7c00, 0xbc00, 0x8000], ids=["nan", "inf", "minus-one", "minus-zero"])
def test_unclean_texels_at_a_corner_an_edge_inside_and_on_a_tile_seam(hip_ctx, bits):
    w, h = TW + 9, TH + 5
    places = [(0, 0), (h - 1, w - 1), (0, 30), (10, 0), (9, w - 1), (7, 20), (TH - 1, TW - 1), (TH, TW), (TH - 1, 10), (12, TW)]
    scene_np = ref.blocky_inputs(w, h, 23)
    for i, (y, x) in enumerate(places):
        scene_np[y, x, i % 3] = bits
    for flags in (0, ref.DENOISE):
        got = _check(hip_ctx, scene_np, dict(flags=flags))
        passed = (got == scene_np).all(-1)
        eligible = ref.eligible(scene_np)
        if bits == 0x8000:  # -0 is clean: every pixel is sharpened
            assert eligible.all() and passed.mean() < 0.05
        else:
            assert passed[~eligible].all() and passed[eligible].mean() < 0.05 and all(not eligible[p] for p in places)
            assert (~eligible).sum() == 3 + 3 + 4 + 4 + 4 + 5 + 5 + 5 + 5 + 5 - 2  # pluses cut by the borders; two pairs of them share a pixel


# ---- stream capture -------------------------------------------------------------------------------------------------------------------------------
def test_captured_call_is_one_kernel_node_and_replays_to_the_same_bytes(fixture):
    import torch
    with side_stream_context() as (ctx, s):
        W, H = gen.WIDTH, gen.HEIGHT
        exposure, settings = gen.CASES[3]
        params = _abi.SharpenParams.default(**settings)
        scene_img, out_img, state = Image(RGBA16F, W, H, None, fixture["scene"]), Image(RGBA16F, W, H), State(exposure)
        before = context_state(ctx)
        torch.cuda.synchronize()
        # the structure of what one call records: a single kernel node, no edges
        hip = hip_runtime()
        stream, graph = C.c_void_p(s.cuda_stream), C.c_void_p()
        assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        try:
            ctx.sharpen(scene_img.plane, state.ptr, out_img.plane, params)
        finally:
            rc = hip.hipStreamEndCapture(stream, C.byref(graph))
        assert rc == 0 and graph.value
        try:
            n_nodes, n_edges = C.c_size_t(0), C.c_size_t(0)
            assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 1
            nodes = (C.c_void_p * 1)()
            kind = C.c_int(-1)
            assert hip.hipGraphGetNodes(graph, nodes, C.byref(n_nodes)) == 0 and hip.hipGraphNodeGetType(C.c_void_p(nodes[0]), C.byref(kind)) == 0
            assert kind.value == 0  # hipGraphNodeTypeKernel
            assert hip.hipGraphGetEdges(graph, None, None, C.byref(n_edges)) == 0 and n_edges.value == 0
        finally:
            assert hip.hipGraphDestroy(graph) == 0
        torch.cuda.synchronize()
        assert out_img.unchanged()  # recording ran nothing
        # one captured call, replayed twice over other scene contents
        replayed = torch.cuda.CUDAGraph()
        with torch.cuda.graph(replayed, stream=s):
            ctx.sharpen(scene_img.plane, state.ptr, out_img.plane, params)
        for seed in (77, 78):
            other = ref.blocky_inputs(W, H, seed, unclean=3)
            scene_img.t.copy_(Image(RGBA16F, W, H, None, other).t)
            out_img.t.fill_(SENTINEL)
            torch.cuda.synchronize()
            replayed.replay()
            torch.cuda.synchronize()
            want = ref.sharpen(other, exposure, settings)
            assert _texels(out_img).tobytes() == want.tobytes(), f"replay with seed {seed}: " + differs(_texels(out_img), want)
            assert out_img.padding_intact() and state.unchanged()
        assert context_state(ctx) == before


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip_ctx, fixture):
    """(tests/test_sharpen_cpu.py runs the whole list on a context without a device; here every kind of it on real planes: the status, and
    out keeps its bytes)"""
    import torch
    W, H = gen.WIDTH, gen.HEIGHT
    scene_img, out_img, state = Image(RGBA16F, W, H, None, fixture["scene"]), Image(RGBA16F, W, H), State(0.5)
    sc, out, st = scene_img.plane, out_img.plane, state.ptr
    P = _abi.SharpenParams.default

    def reshaped(plane, **kw):
        a = dict(ptr=plane.ptr, width=plane.width, height=plane.height, row_pitch_bytes=plane.row_pitch_bytes)
        a.update(kw)
        return _abi.Plane(a["ptr"], a["width"], a["height"], a["row_pitch_bytes"], RGBA16F)
    INVALID, FORMAT = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
    nan, inf = float("nan"), float("inf")
    cases = [((retyped(sc, _abi.FORMAT_R32_SFLOAT), st, out, P()), FORMAT), ((sc, st, retyped(out, _abi.FORMAT_R8G8B8A8_UNORM), P()), FORMAT),
             ((reshaped(sc, ptr=None), st, out, P()), INVALID), ((sc, st, reshaped(out, ptr=None), P()), INVALID),
             ((reshaped(sc, width=0), st, reshaped(out, width=0), P()), INVALID), ((reshaped(sc, height=0), st, reshaped(out, height=0), P()), INVALID),
             ((sc, st, reshaped(out, width=W - 1), P()), INVALID), ((sc, st, reshaped(out, height=H - 1), P()), INVALID),
             ((sc, st, reshaped(out, row_pitch_bytes=W * 8 - 4), P()), INVALID), ((reshaped(sc, row_pitch_bytes=W * 8 - 8), st, out, P()), INVALID),
             ((sc, st, reshaped(out, ptr=out.ptr + 2), P()), INVALID), ((reshaped(sc, ptr=sc.ptr + 1), st, out, P()), INVALID),
             ((sc, st, reshaped(out, row_pitch_bytes=W * 8 + 2), P()), INVALID),
             ((sc, st + 2, out, P()), INVALID), ((sc, st + 1, out, P()), INVALID),
             ((sc, st, out, P(), (9, 3)), INVALID), ((sc, st, out, P(), (0, H + 1)), INVALID), ((sc, st, out, P(), (H + 1, H + 1)), INVALID),
             ((sc, st, out, P(sharpness=-0.001)), INVALID), ((sc, st, out, P(sharpness=1.001)), INVALID), ((sc, st, out, P(sharpness=nan)), INVALID),
             ((sc, st, out, P(pre_scale=0.0)), INVALID), ((sc, st, out, P(pre_scale=-1.0)), INVALID), ((sc, st, out, P(pre_scale=inf)), INVALID),
             ((sc, st, out, P(pre_scale=nan)), INVALID),
             ((sc, st, out, P(flags=2)), INVALID), ((sc, st, out, P(flags=0x80000001)), INVALID),
             ((sc, st, sc, P()), INVALID),                                            # in place
             ((sc, st, reshaped(out, ptr=sc.ptr + W * 8), P()), INVALID),             # out begins inside the scene
             ((reshaped(sc, ptr=out.ptr + 8), st, out, P()), INVALID),                # the scene begins inside out
             ((sc, out.ptr + 32, out, P()), INVALID),                                 # the exposure inside out
             ((sc, out.ptr - 12, out, P()), INVALID)]                                 # the exposure ends inside out
    for args, status in cases:
        with pytest.raises(lib.SahError) as e:
            hip_ctx.sharpen(*args)
        assert e.value.status == status, args
    for args in ((None, st, out, P()), (sc, st, None, P()), (sc, st, out, None)):  # NULL scene, out, params: below the wrapper's byref
        L = hip_ctx.lib
        ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
        assert L.sah_sharpen(hip_ctx.handle, ref_of(args[0]), C.c_void_p(args[1]), ref_of(args[2]), ref_of(args[3]), 0, 0) == INVALID
    torch.cuda.synchronize()
    assert out_img.unchanged() and scene_img.unchanged() and state.unchanged()


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------------
EXTENTS = [(80, 36), (45, 50), (45, 50)]
FRAME_SETTINGS = [dict(sharpness=1.0, pre_scale=1.0, flags=0), dict(sharpness=0.5, pre_scale=1.0, flags=ref.DENOISE), dict(sharpness=0.25, pre_scale=0.5, flags=ref.DENOISE)]
FRAME_EXPOSURES = [None, 0.375, None]


def _frames(seed):
    return [ref.blocky_inputs(w, h, seed + i, unclean=3) for i, (w, h) in enumerate(EXTENTS)]


def test_frames_of_two_extents_through_the_python_wrapper(hip_ctx):
    import torch
    frames = _frames(900)
    sharpener = frame.Sharpener(hip_ctx, *EXTENTS[0])
    assert sharpener.params.sharpness == 1.0 and sharpener.params.pre_scale == 1.0 and sharpener.params.flags == 0  # the header's defaults
    planes = []
    for sc, settings, exposure in zip(frames, FRAME_SETTINGS, FRAME_EXPOSURES):
        sharpener.params = _abi.SharpenParams.default(**settings)
        state = State(exposure)
        out = sharpener.sharpen(util.to_torch(sc), state.ptr)
        torch.cuda.synchronize()
        assert out is sharpener.sharpened and tuple(out.shape) == sc.shape
        got, want = out.cpu().numpy().view(np.uint16), ref.sharpen(sc, exposure, settings)
        assert got.tobytes() == want.tobytes(), differs(got, want)
        planes.append(out)
    assert planes[0] is not planes[1] and planes[1] is planes[2]  # re-created for another extent, kept while it stays
    assert frame.Sharpener(hip_ctx, 8, 8, sharpness=0.5, flags=1).params.flags == 1


def test_frames_of_two_extents_through_the_cpp_facade(tmp_path):
    frames = _frames(950)
    stops = [0.0, 1.0, 2.0]  # SharpenSettings::from_stops: sharpness 1, 0.5, 0.25
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(frames)], np.uint32).tobytes())
        for sc, settings, exposure, st in zip(frames, FRAME_SETTINGS, FRAME_EXPOSURES, stops):
            assert 2.0 ** -st == settings["sharpness"]
            f.write(np.array([sc.shape[1], sc.shape[0], settings["flags"] & ref.DENOISE, exposure is not None], np.uint32).tobytes())
            f.write(np.array([st, settings["pre_scale"], exposure or 0.0], f32).tobytes() + sc.tobytes())
    subprocess.check_call([host_program("host_sharpen", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    at = 0
    for i, (sc, settings, exposure) in enumerate(zip(frames, FRAME_SETTINGS, FRAME_EXPOSURES)):
        got = np.frombuffer(blob[at:at + sc.nbytes], np.uint16).reshape(sc.shape)
        at += sc.nbytes
        want = ref.sharpen(sc, exposure, settings)
        assert got.tobytes() == want.tobytes(), f"frame {i}: " + differs(got, want)
    assert at == len(blob)
