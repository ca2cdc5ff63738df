"""GPU: sah_taa_upscale (include/sah_taa_upscale.h) against the numpy restatement (tests/taa_upscale_ref.py) and its committed fixture, bit
for bit; the Python TemporalUpscaler and the C++ façade's TemporalUpscaling over successive frames; and a rendered frame end to end.  The
kernel's tile is 64 x 16 output pixels."""
import faulthandler
import math
import os
import subprocess

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, images, lib, mesh, scene
from tests import mv_reproject, taa_ref, util
from tests import taa_upscale_ref as ref
from tests.host_programs import host_program
from tests.support import context_state, differs, Image, resized, retyped, side_stream_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "taa_upscale_89x23_to_133x35.npz")
RENDER, OUTPUT = (89, 23), (133, 35)
RGBA16F, D32, RG16F = _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16_SFLOAT
HDR, NO_HISTORY = _abi.TAA_HDR_WEIGHTS, _abi.TAA_HISTORY_INVALID


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)  # each test under a limit of its own: an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


def _params(blend, min_confidence, jitter, previous_jitter, flags):
    p = _abi.TaaUpscaleParams()
    p.blend, p.min_confidence, p.flags = blend, min_confidence, flags
    p.jitter[:] = [float(v) for v in jitter]
    p.previous_jitter[:] = [float(v) for v in previous_jitter]
    return p


def _fixture_params(fx, flags):
    return _params(float(fx["blend"]), float(fx["min_confidence"]), fx["jitter"], fx["previous_jitter"], flags)


def _fixture_ref(fx, flags, **replace):
    a = {k: fx[k] for k in ("lit", "depth", "motion_vectors", "history")}
    a.update(replace)
    return ref.upscale(a["lit"], a["depth"], a["motion_vectors"], a["history"], OUTPUT, float(fx["blend"]), float(fx["min_confidence"]), fx["jitter"],
                       fx["previous_jitter"], flags)


class Planes:
    """the five device planes of one call; pitches / offsets in the order lit, depth, motion vectors, history, out"""

    def __init__(self, lit, depth, mv, history, output, pitches=(None,) * 5, offsets=(0,) * 5, out=None):
        h, w = depth.shape
        self.W, self.H = output
        self.lit = Image(RGBA16F, w, h, pitches[0], lit, offsets[0])
        self.depth = Image(D32, w, h, pitches[1], depth, offsets[1])
        self.mv = Image(RG16F, w, h, pitches[2], mv, offsets[2])
        self.history = None if history is None else Image(RGBA16F, self.W, self.H, pitches[3], history, offsets[3])
        self.out = out or Image(RGBA16F, self.W, self.H, pitches[4], None, offsets[4])

    def resolve(self, ctx, params, rows=(0, 0)):
        import torch
        ctx.taa_upscale(self.lit.plane, self.depth.plane, self.mv.plane, None if self.history is None else self.history.plane, self.out.plane, params, rows)
        torch.cuda.synchronize()
        assert self.lit.unchanged() and self.depth.unchanged() and self.mv.unchanged() and (self.history is None or self.history.unchanged())
        return self.out.texels(np.uint16).reshape(self.H, self.W, 4)


def _fixture_planes(fx, **kw):
    return Planes(fx["lit"], fx["depth"], fx["motion_vectors"], fx["history"], OUTPUT, **kw)


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,key", [(0, "out_plain"), (HDR, "out_hdr")])
def test_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture, flags, key):
    fx = fixture
    got = _fixture_planes(fx).resolve(hip_ctx, _fixture_params(fx, flags))
    assert np.array_equal(got, fx[key]), differs(got, fx[key])
    again = _fixture_planes(fx).resolve(hip_ctx, _fixture_params(fx, flags))
    assert again.tobytes() == got.tobytes()


def test_without_history_the_output_is_the_restatements_upsample(hip_ctx, fixture):
    fx = fixture
    want = fx["out_no_history"]
    assert np.array_equal(want, _fixture_ref(fx, NO_HISTORY | HDR, history=None))
    for history in (None, fx["history"]):  # not read, given or not
        got = Planes(fx["lit"], fx["depth"], fx["motion_vectors"], history, OUTPUT).resolve(hip_ctx, _fixture_params(fx, NO_HISTORY | HDR))
        assert np.array_equal(got, want), differs(got, want)


@pytest.mark.parametrize("extents", ref.EXTENTS, ids=lambda e: f"{e[0][0]}x{e[0][1]}-{e[1][0]}x{e[1][1]}")
@pytest.mark.parametrize("flags", [0, HDR])
def test_small_extents(hip_ctx, extents, flags):
    (w, h), (W, H) = extents
    lit, depth, mv, _ = taa_ref.random_inputs(w, h, 11 + w + W)
    history = taa_ref.random_inputs(W, H, 12 + w + W)[3]
    previous = (-0.25, 0.4)
    blended = 0
    for jitter in ((0.0, 0.0), (0.5, -0.5), (0.25, 0.25)):
        got = Planes(lit, depth, mv, history, (W, H)).resolve(hip_ctx, _params(0.1, 0.05, jitter, previous, flags))
        want, info = ref.upscale_ex(lit, depth, mv, history, (W, H), 0.1, 0.05, jitter, previous, flags)
        assert np.array_equal(got, want), f"jitter {jitter}: " + differs(got, want)
        blended += int((~info["fallback"]).sum())
    if W * H >= 64:
        assert blended > 0


# pitches and offsets in bytes: lit, depth, motion vectors, history, out
@pytest.mark.parametrize("pitches,offsets", [((89 * 8 + 4, 89 * 4 + 12, 89 * 4 + 20, 133 * 8 + 12, 133 * 8 + 4), (4, 8, 12, 4, 12)),  # no plane 16-byte aligned
                                             ((720, 368, 384, 1072, 1088), (0, 0, 16, 32, 0)),                                          # padded, all 16-byte aligned: the 16-byte path
                                             ((720, 368, 384, 1072, 1088), (0, 0, 0, 8, 0))])                                           # one plane 8-byte aligned only
def test_pitches_offsets_sentinels_and_inputs(hip_ctx, fixture, pitches, offsets):
    fx = fixture
    p = _fixture_planes(fx, pitches=pitches, offsets=offsets)
    got = p.resolve(hip_ctx, _fixture_params(fx, HDR))  # (asserts the inputs unchanged)
    assert np.array_equal(got, fx["out_hdr"]), differs(got, fx["out_hdr"])
    assert p.out.padding_intact()


def test_row_bands_compose_to_the_whole_from_the_render_rows_the_header_names(hip_ctx, fixture):
    """Bands that split inside a tile (9) and on tile edges (16, 32); each band's call sees only the render rows the header says it reads,
    every other row of lit, depth and motion_vectors is NaN."""
    fx = fixture
    (w, h), (W, H), pitch = RENDER, OUTPUT, 1072
    out = Image(RGBA16F, W, H, pitch)
    for rows in ((9, 16), (0, 9), (32, H), (16, 32)):
        first, last = ref.render_rows_read(rows[0], rows[1], H, h, float(fx["jitter"][1]))
        assert last - first + 1 < h
        lit, depth, mv = fx["lit"].copy(), fx["depth"].copy(), fx["motion_vectors"].copy()
        for plane, poison in ((lit, 0x7e00), (depth.view(np.uint32), 0x7fc00000), (mv, 0x7e00)):
            plane[:first] = poison
            plane[last + 1:] = poison
        p = Planes(lit, depth, mv, fx["history"], OUTPUT, out=out)
        before = out.bytes().copy()
        p.resolve(hip_ctx, _fixture_params(fx, HDR), rows)
        changed = out.bytes() != before
        body = changed[:H * pitch].reshape(H, pitch)
        assert not body[:rows[0]].any() and not body[rows[1]:].any() and not body[:, W * 8:].any() and not changed[H * pitch:].any()
    got = out.texels(np.uint16).reshape(H, W, 4)
    assert np.array_equal(got, fx["out_hdr"]), differs(got, fx["out_hdr"])
    before = out.bytes().copy()
    _fixture_planes(fx, out=out).resolve(hip_ctx, _fixture_params(fx, 0), (5, 5))  # an empty band writes nothing
    assert (out.bytes() == before).all()


def test_rows_beyond_2_to_28_where_a_tiles_footprint_outgrows_the_staged_cells(hip_ctx):
    """From 2^28 on float(Y) moves in steps of 32, so the nearest texels of a 16-row tile can lie 32 rows apart: more than the 19 staged rows.
    Such a tile gathers its taps from memory instead (taa_upscale.hip).  A 1 x (2^28 + 48) image at scale 1, zero but for its last rows, the
    band from 2^28 - 32 to the end: tiles on both sides of 2^28, restated through a window of the image."""
    import torch
    H = h = (1 << 28) + 48
    band, first = ((1 << 28) - 32, H), (1 << 28) - 256  # `first`: where the non-zero rows of every plane begin
    tail = H - first
    lit, depth, mv, _ = taa_ref.random_inputs(1, tail, 31, specials=False)
    history = taa_ref.random_inputs(1, tail, 32, specials=False)[3]
    jitter, previous = (0.25, -0.125), (-0.25, 0.375)
    mv.view(np.float16)[..., 0] = 0.5  # with dj.x = -0.5: no motion in x, the image being one pixel wide
    _, j = ref.sample_positions(H, h, jitter[1], band[0], band[1] - band[0])
    starts = np.arange(0, band[1] - band[0], ref.TILE[1])
    spans = j[np.minimum(starts + ref.TILE[1], len(j)) - 1] - j[starts] + 3
    assert spans.max() > ref.FOOTPRINT[1] and spans.min() <= ref.FOOTPRINT[1]  # tiles of both kinds
    planes, tensors = {}, []
    for name, data, fmt, channels, dtype in (("lit", lit, RGBA16F, 4, torch.int16), ("depth", depth, D32, 0, torch.float32), ("mv", mv, RG16F, 2, torch.int16),
                                             ("history", history, RGBA16F, 4, torch.int16), ("out", None, RGBA16F, 4, torch.int16)):
        t = torch.zeros((H, 1) + ((channels,) if channels else ()), dtype=dtype, device="cuda")
        if data is not None:
            t[first:] = torch.from_numpy(data.view(np.int16) if channels else data).cuda()
        tensors.append(t)
        planes[name] = _abi.Plane(t.data_ptr(), 1, H, _abi.FORMAT_BPP[fmt], fmt)
    out_t = tensors[-1]
    try:
        for flags in (0, HDR):
            out_t.zero_()
            hip_ctx.taa_upscale(planes["lit"], planes["depth"], planes["mv"], planes["history"], planes["out"], _params(0.25, 0.05, jitter, previous, flags), band)
            torch.cuda.synchronize()
            got = out_t[band[0]:].cpu().numpy().view(np.uint16)
            want, info = ref.upscale_ex(lit, depth, mv, history, (1, H), 0.25, 0.05, jitter, previous, flags,
                                        window=(band[0], band[1] - band[0], first, h, first))
            assert np.array_equal(got, want), f"flags {flags}: " + differs(got, want)
            assert (~info["fallback"]).mean() > 0.5 and not out_t[band[0] - 64:band[0]].any()
    finally:
        del tensors, out_t, t
        torch.cuda.empty_cache()


# ---- sequences ------------------------------------------------------------------------------------------------------------------------------
def _sequence(frames, w, h, seed):
    return [taa_ref.random_inputs(w, h, seed + i, specials=(i % 3 == 1))[:3] for i in range(frames)]


def _restated_sequence(seq, jitters, output, blend, min_confidence, hdr):
    outs, history, previous = [], None, None
    for n, (lit, depth, mv) in enumerate(seq):
        j = jitters[n % len(jitters)]
        flags = (HDR if hdr else 0) | (NO_HISTORY if history is None else 0)
        history = ref.upscale(lit, depth, mv, history, output, blend, min_confidence, j, j if previous is None else previous, flags)
        previous = j
        outs.append(history)
    return outs


def test_eight_frames_of_ping_pong_match_the_restatement_frame_by_frame(hip_ctx):
    import torch
    (w, h), (W, H), blend, mc = (64, 36), (96, 54), 0.1, 0.05
    seq, jitters = _sequence(8, w, h, 300), ref.upscale_jitter_cycle(W, w)
    want = _restated_sequence(seq, jitters, (W, H), blend, mc, True)
    upscaler = frame.TemporalUpscaler(hip_ctx, render=(w, h), output=(W, H), blend=blend, min_confidence=mc, hdr_weights=True)
    for n, (lit, depth, mv) in enumerate(seq):
        out = upscaler.resolve(util.to_torch(lit), torch.from_numpy(depth).cuda(), util.to_torch(mv), jitters[n])
        torch.cuda.synchronize()
        got = util.from_torch(out, np.uint16)
        assert np.array_equal(got, want[n]), f"frame {n}: " + differs(got, want[n])
    first = ref.upscale(*seq[0], None, (W, H), blend, mc, jitters[0], jitters[0], NO_HISTORY)
    assert np.array_equal(want[0], first) and not np.array_equal(want[7], ref.upscale(*seq[7], None, (W, H), blend, mc, jitters[7], jitters[7], NO_HISTORY))
    # after a cut the next frame is the upsample again
    upscaler.reset()
    out = upscaler.resolve(util.to_torch(seq[3][0]), torch.from_numpy(seq[3][1]).cuda(), util.to_torch(seq[3][2]), jitters[0])
    torch.cuda.synchronize()
    assert np.array_equal(util.from_torch(out, np.uint16), ref.upscale(*seq[3], None, (W, H), blend, mc, jitters[0], jitters[0], NO_HISTORY))


def test_three_frames_through_the_cpp_facade_match_the_python_upscaler(tmp_path, hip_ctx):
    import torch
    (W, H), scale, blend, mc = (96, 54), 1.5, 0.25, 0.05
    w, h = ref.render_resolution((W, H), scale)
    assert (w, h) == (64, 36)
    seq, jitters = _sequence(3, w, h, 500), ref.upscale_jitter_cycle(W, w)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([W, H, 3, 1], np.uint32).tobytes())
        f.write(np.array([blend, mc, scale], np.float32).tobytes())
        for lit, depth, mv in seq:
            f.write(lit.tobytes() + depth.tobytes() + mv.tobytes())
    subprocess.check_call([host_program("host_taa_upscale", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    assert np.frombuffer(blob[:12], np.uint32).tolist() == [w, h, len(jitters)] and len(jitters) == 18
    blob, size = blob[12:], 8 + W * H * 8
    assert len(blob) == 3 * size
    upscaler = frame.TemporalUpscaler(hip_ctx, render=(w, h), output=(W, H), blend=blend, min_confidence=mc, hdr_weights=True)
    want = _restated_sequence(seq, jitters, (W, H), blend, mc, True)
    for n, (lit, depth, mv) in enumerate(seq):
        jitter = np.frombuffer(blob[n * size:n * size + 8], np.float32)
        assert jitter.tobytes() == np.array(jitters[n], np.float32).tobytes(), f"frame {n}: the façade's jitter {jitter} is not {jitters[n]}"
        facade = np.frombuffer(blob[n * size + 8:(n + 1) * size], np.uint16).reshape(H, W, 4)
        out = upscaler.resolve(util.to_torch(lit), torch.from_numpy(depth).cuda(), util.to_torch(mv), jitters[n])
        torch.cuda.synchronize()
        got = util.from_torch(out, np.uint16)
        assert np.array_equal(facade, got), f"frame {n}: " + differs(facade, got)
        assert np.array_equal(got, want[n])


# ---- the call contract ----------------------------------------------------------------------------------------------------------------------
def test_side_stream_without_host_sync_and_under_capture(fixture):
    import torch
    fx = fixture
    (w, h), (W, H) = RENDER, OUTPUT
    with side_stream_context() as (ctx, s):
        a = _fixture_planes(fx)
        second = Image(RGBA16F, W, H)
        blend, mc = float(fx["blend"]), float(fx["min_confidence"])
        p1, p2 = _fixture_params(fx, HDR), _params(blend, mc, fx["previous_jitter"], fx["jitter"], 0)
        want2 = ref.upscale(fx["lit"], fx["depth"], fx["motion_vectors"], fx["out_hdr"], OUTPUT, blend, mc, fx["previous_jitter"], fx["jitter"], 0)

        def two_frames():  # the second call's history is the first call's output: no host synchronisation in between
            ctx.taa_upscale(a.lit.plane, a.depth.plane, a.mv.plane, a.history.plane, a.out.plane, p1)
            ctx.taa_upscale(a.lit.plane, a.depth.plane, a.mv.plane, a.out.plane, second.plane, p2)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            two_frames()
        s.synchronize()
        assert np.array_equal(a.out.texels(np.uint16).reshape(H, W, 4), fx["out_hdr"])
        assert np.array_equal(second.texels(np.uint16).reshape(H, W, 4), want2)
        # one captured graph, a linear chain; replayed over other input contents
        lit2, depth2, mv2, _ = taa_ref.random_inputs(w, h, 77)
        history2 = taa_ref.random_inputs(W, H, 78)[3]
        b = Planes(lit2, depth2, mv2, history2, OUTPUT)
        direct1 = ref.upscale(lit2, depth2, mv2, history2, OUTPUT, blend, mc, fx["jitter"], fx["previous_jitter"], HDR)
        direct2 = ref.upscale(lit2, depth2, mv2, direct1, OUTPUT, blend, mc, fx["previous_jitter"], fx["jitter"], 0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            two_frames()
        for dst, src in ((a.lit, b.lit), (a.depth, b.depth), (a.mv, b.mv), (a.history, b.history)):
            dst.t.copy_(src.t)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(a.out.texels(np.uint16).reshape(H, W, 4), direct1)
        assert np.array_equal(second.texels(np.uint16).reshape(H, W, 4), direct2)
        assert not np.array_equal(direct2, want2)


def test_no_side_effects_on_the_context(hip_ctx, fixture):
    fx = fixture
    f = util.LightingFrame(64, 36, seed=5, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flavour="atrium")
    f.run_hip(hip_ctx)

    def state():
        return context_state(hip_ctx)
    before = state()
    got = _fixture_planes(fx).resolve(hip_ctx, _fixture_params(fx, 0))
    assert state() == before
    assert np.array_equal(got, fx["out_plain"])


def test_refusals_launch_nothing(hip_ctx, fixture):
    """(tests/test_taa_upscale_cpu.py runs the whole list on a context without a device; here: the target keeps its bytes)"""
    import torch
    fx = fixture
    (w, h), (W, H) = RENDER, OUTPUT
    p = _fixture_planes(fx)
    ok = _fixture_params(fx, 0)
    lit, depth, mv, history, out = p.lit.plane, p.depth.plane, p.mv.plane, p.history.plane, p.out.plane
    blend = float(fx["blend"])

    INVALID, FORMAT = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
    cases = [((lit, depth, mv, history, retyped(out, _abi.FORMAT_R32_SFLOAT), ok), FORMAT),
             ((lit, retyped(depth, _abi.FORMAT_R32_SFLOAT), mv, history, out, ok), FORMAT),
             ((lit, depth, mv, None, out, ok), INVALID),
             ((lit, depth, mv, history, out, ok, (0, H + 1)), INVALID),
             ((lit, depth, mv, history, out, ok, (9, 3)), INVALID),
             ((lit, depth, mv, history, out, _fixture_params(fx, 4)), INVALID),
             ((lit, depth, mv, history, out, _params(0.0, 0.05, (0, 0), (0, 0), 0)), INVALID),
             ((lit, depth, mv, history, out, _params(blend, -0.01, (0, 0), (0, 0), 0)), INVALID),
             ((lit, depth, mv, history, out, _params(blend, float("nan"), (0, 0), (0, 0), 0)), INVALID),
             ((lit, depth, mv, history, out, _params(0.5, 0.05, (float("nan"), 0), (0, 0), 0)), INVALID),
             ((lit, depth, mv, out, out, ok), INVALID),
             ((lit, depth, mv, history, resized(out, W - 1, H), ok), INVALID),                              # history and out differ
             ((lit, resized(depth, w - 1, h), mv, history, out, ok), INVALID),                               # the render planes differ
             ((lit, depth, mv, resized(history, w - 1, h), resized(out, w - 1, h), ok), INVALID),           # downscaling in x
             ((lit, depth, mv, None, resized(out, W, h - 1), _fixture_params(fx, NO_HISTORY)), INVALID)]    # downscaling in y, no history
    for args, status in cases:
        with pytest.raises(lib.SahError) as e:
            hip_ctx.taa_upscale(*args)
        assert e.value.status == status, args
    torch.cuda.synchronize()
    assert p.out.unchanged()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def test_rendered_frames_end_to_end(hip_ctx):
    """The atrium at 128 x 72 through sah_gbuffer_motion_render and sah_lighting for two views of a camera that stands still and changes its
    jitter, upscaled to 192 x 108: the output is the restatement's on the device's own planes; with the jitter taken out the history is read
    where the output pixel is — |q - centre| within rx times the bound tests/test_taa_gpu.py uses (DEVIATION_FACTOR x FIXTURE_EXCESS_PIXELS,
    what the motion vectors are allowed against the fp64 reprojection, plus half an fp16 spacing below 1), over the SOLID-covered pixels but
    MAX_LEFT_OUT of them; and sah_bloom and sah_tonemap take the result at the output resolution."""
    import torch
    (w, h), (W, H), blend, mc = (128, 72), (192, 108), 0.1, 0.05
    j0, j1 = (0.3, -0.2), (-0.25, 0.4)
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    view = scene.SceneView()
    view.rotate(0.0, math.radians(90.0))
    view.set_position([-7.0, 1.0, 0.0])
    view.set_render_resolution(w, h)
    view.set_perspective_projection(75.0, float(w) / float(h), 0.05)
    upscaler = frame.TemporalUpscaler(hip_ctx, render=(w, h), output=(W, H), blend=blend, min_confidence=mc, hdr_weights=True)
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    frames = []
    for jitter in (j0, j1):
        view.jitter = np.array(jitter, np.float32)
        view.update_transforms()
        gb = {k: torch.zeros((h, w) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
        mv = torch.zeros((h, w, 2), dtype=torch.int16, device="cuda")
        frame.rasterised_frame(hip_ctx, geo, view.gpu_data, gb, motion_vectors=mv, fused_motion=True)
        torch.cuda.synchronize()
        gb_np = {k: v.cpu().numpy() for k, v in gb.items()}
        gb_np["normals"] = gb_np["normals"].view(np.uint16)
        inputs = frame.LightingInputs(w, h, gbuffer=gb_np, seed=3, sun_mode=_abi.SHADOW_MODE_RT, gi=_abi.GI_NONE)
        inputs.view = view
        lit = inputs.run_hip(hip_ctx)
        out = upscaler.resolve(util.to_torch(lit), gb["depth"], mv, jitter)
        torch.cuda.synchronize()
        frames.append((lit, gb_np["depth"], util.from_torch(mv, np.uint16), util.from_torch(out, np.uint16), out))
    (lit0, depth0, mv0, out0, _), (lit1, depth1, mv1, out1, out1_t) = frames
    want0 = ref.upscale(lit0, depth0, mv0, None, (W, H), blend, mc, j0, j0, HDR | NO_HISTORY)
    assert np.array_equal(out0, want0), differs(out0, want0)
    want, info = ref.upscale_ex(lit1, depth1, mv1, out0, (W, H), blend, mc, j1, j0, HDR)
    assert np.array_equal(out1, want), differs(out1, want)
    assert info["valid"].mean() > 0.9 and (~info["fallback"]).mean() > 0.9
    solid = depth1[info["j"]][:, info["i"]] > 0
    assert solid.mean() > 0.5
    centre = np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), -1)
    off = np.abs(info["q"].astype(np.float64) - centre).max(-1)
    bound = (W / w) * (mv_reproject.DEVIATION_FACTOR * mv_reproject.FIXTURE_EXCESS_PIXELS + 2.0 ** -12)
    left_out = (off[solid] > bound).mean()
    print(f"end to end: {float(solid.mean()):.2f} of the pixels SOLID-covered, max |q - centre| {float(off[solid].max()):.5f} (bound {bound:.5f}), "
          f"{float(left_out):.4f} left out")
    assert left_out <= mv_reproject.MAX_LEFT_OUT
    # the post chain takes the upscaled frame at the output resolution
    mips = [torch.zeros((mh, mw, 4), dtype=torch.int16, device="cuda") for (mw, mh) in images.bloom_mip_sizes(W, H, 6)]
    final = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    scene_plane, chain = images.plane(out1_t, RGBA16F), images.mipchain(mips)
    hip_ctx.bloom(scene_plane, chain)
    hip_ctx.tonemap(scene_plane, chain, images.plane(final, _abi.FORMAT_R8G8B8A8_SRGB))
    torch.cuda.synchronize()
    assert int(final.cpu().numpy()[..., :3].max()) > 0 and np.array_equal(util.from_torch(out1_t, np.uint16), out1)
