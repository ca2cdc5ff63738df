"""GPU: sah_exposure_meter and sah_exposure_apply (include/sah_exposure.h) against the numpy restatement (tests/exposure_ref.py) run on the
device's own planes, and the committed fixture, bit for bit: histogram words, states and exposed planes; the Python AutoExposure and the
C++ façade's AutoExposure over successive frames; and the frame the pass exists for — the rasterised atrium lit in LPV mode with the sun as
it is and eight times brighter, exposed, bloomed and tonemapped.  The kernel's tile is 128 x 4 pixels (a wave per row of it, two pixels
per lane), the grid persistent: max_workgroups below the number of tiles makes a workgroup loop, and more than one workgroup exercises
the ticket."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, images, lib, mesh, scene
from tests import exposure_ref as ref
from tests import util
from tests.host_programs import host_program
from tests.support import context_state, differs, Image, retyped, same, SENTINEL, side_stream_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_exposure as gen  # noqa: E402

f32 = np.float32
RGBA16F = _abi.FORMAT_R16G16B16A16_SFLOAT
CUT = _abi.EXPOSURE_HISTORY_INVALID
TILES_3X3 = (3 * ref.TILE[0], 3 * ref.TILE[1])


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)  # each test under a limit of its own: an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fixture():
    fx = np.load(gen.FIXTURE)
    scene_np = np.ascontiguousarray(fx["scene_plane"][:, :gen.WIDTH])
    return {"scene": scene_np, "frames": gen.frames(scene_np), "histograms": fx["histograms"], "states": fx["states"], "exposed": fx["exposed"]}


def _params(**changes):
    return _abi.ExposureParams.default(**changes)


class Buffers:
    """`work` and two states in one device allocation, sentinel bytes everywhere else"""
    WORK, STATES, SIZE = 64, (1280, 1344), 2048

    def __init__(self, work_offset=0, states=None):
        import torch
        host = np.full(self.SIZE, SENTINEL, np.uint8)
        for i, s in enumerate(states or ()):
            if s is not None:
                host[self.STATES[i]:self.STATES[i] + 16] = np.frombuffer(np.asarray(s, ref.STATE).tobytes(), np.uint8)
        self.host_in = host.copy()
        self.t = torch.from_numpy(host).cuda()
        self.work_at = self.WORK + work_offset
        self.work = self.t.data_ptr() + self.work_at

    def state_ptr(self, i):
        return None if i is None else self.t.data_ptr() + self.STATES[i]

    def bytes(self):
        return self.t.cpu().numpy()

    def histogram(self):
        return self.bytes()[self.work_at:self.work_at + 1024].view(np.uint32).copy()

    def state(self, i):
        return self.bytes()[self.STATES[i]:self.STATES[i] + 16].view(ref.STATE)[0].copy()

    def intact(self, written_states=()):
        """no byte outside `work` and the states named changed"""
        b, mask = self.bytes(), np.ones(self.SIZE, bool)
        mask[self.work_at:self.work_at + lib.EXPOSURE_WORK_BYTES] = False
        for i in written_states:
            mask[self.STATES[i]:self.STATES[i] + 16] = False
        return bool((b[mask] == self.host_in[mask]).all())

    def unchanged(self):
        return bool((self.bytes() == self.host_in).all())


def _scene_image(scene_np, pitch=None, offset=0):
    h, w = scene_np.shape[:2]
    return Image(RGBA16F, w, h, pitch, scene_np, offset)


def _texels(img):
    return img.texels(np.uint16).reshape(img.h, img.w, 4)


def _meter(ctx, scene_img, buffers, state_in, state_out, out_img, params):
    import torch
    ctx.exposure_meter(scene_img.plane, buffers.state_ptr(state_in), buffers.state_ptr(state_out), buffers.work, None if out_img is None else out_img.plane, params)
    torch.cuda.synchronize()


def _check_meter(ctx, scene_np, settings, state_in=None, fused=True, pitches=(None, None), offsets=(0, 0), in_place=False, work_offset=0):
    """one call against the restatement: histogram, state_out, exposed plane, sentinels; returns (histogram, state, exposed)"""
    h, w = scene_np.shape[:2]
    cut = bool(settings.get("flags", 0) & CUT)
    buffers = Buffers(work_offset, [state_in, None])
    scene_img = _scene_image(scene_np, pitches[0], offsets[0])
    out_img = None if not fused else (scene_img if in_place else Image(RGBA16F, w, h, pitches[1], None, offsets[1]))
    _meter(ctx, scene_img, buffers, None if cut else 0, 1, out_img, _params(**settings))
    want_n, want_state = ref.meter(scene_np, state_in, settings)
    got_n, got_state = buffers.histogram(), buffers.state(1)
    assert same(got_n, want_n), "histogram: " + differs(got_n, want_n)
    assert same(got_state, want_state), f"state {got_state} != {want_state}"
    assert buffers.intact((1,)), "bytes around work or the states changed"
    exposed = None
    if fused:
        exposed, want = _texels(out_img), ref.apply(scene_np, state_in["exposure"])
        assert same(exposed, want), "exposed: " + differs(exposed, want)
        assert out_img.padding_intact()
    if not in_place:
        assert scene_img.unchanged()
    return got_n, got_state, exposed


PREVIOUS = np.array((0.375, -1.5, 11, 7), ref.STATE)


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
def _fixture_sequence(ctx, fixture):
    import torch
    p = dict(gen.PARAMS)
    buffers = Buffers()
    out = []
    for i, sc in enumerate(fixture["frames"]):
        scene_img, out_img = _scene_image(sc), Image(RGBA16F, gen.WIDTH, gen.HEIGHT)
        new = i % 2
        if i == 0:
            _meter(ctx, scene_img, buffers, None, new, None, _params(**dict(p, flags=CUT)))
            ctx.exposure_apply(scene_img.plane, buffers.state_ptr(new), out_img.plane)
            torch.cuda.synchronize()
        else:
            _meter(ctx, scene_img, buffers, 1 - new, new, out_img, _params(**p))
        out.append((buffers.histogram(), buffers.state(new), _texels(out_img)))
        assert scene_img.unchanged() and out_img.padding_intact()
    return out


def test_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture):
    got = _fixture_sequence(hip_ctx, fixture)
    for i, (n, state, exposed) in enumerate(got):
        assert same(n, fixture["histograms"][i]), f"frame {i}, histogram: " + differs(n, fixture["histograms"][i])
        assert same(state, fixture["states"][i]), f"frame {i}: state {state} != {fixture['states'][i]}"
        assert same(exposed, fixture["exposed"][i]), f"frame {i}, exposed: " + differs(exposed, fixture["exposed"][i])
    again = _fixture_sequence(hip_ctx, fixture)
    assert all(same(a, b) for x, y in zip(got, again) for a, b in zip(x, y))


# ---- extents --------------------------------------------------------------------------------------------------------------------------------
# tile 128 x 4: one below, at and one above it in each dimension; odd widths end a row on the single-pixel tail of a lane; three tiles by three
@pytest.mark.parametrize("extent", [(1, 1), (2, 3), (3, 1), (127, 3), (128, 4), (129, 5), (127, 5), (129, 3), (255, 8), TILES_3X3])
def test_extents(hip_ctx, extent):
    w, h = extent
    scene_np = ref.random_inputs(w, h, 11 * w + h)
    _check_meter(hip_ctx, scene_np, dict(adaptation=0.5), PREVIOUS)
    n, state, _ = _check_meter(hip_ctx, scene_np, dict(flags=CUT), fused=False)
    if w * h >= 64:
        L = ref.luminance(scene_np)
        assert 0 < int(n.sum()) < w * h and np.isnan(L).any() and (L < 0).any() and state["window"] > 0  # uncounted pixels are there, and it metered


# ---- pitches and alignment ----------------------------------------------------------------------------------------------------------------
# pitches and offsets in bytes: scene, exposed_out
@pytest.mark.parametrize("pitches,offsets", [((69 * 8 + 4, 69 * 8 + 12), (4, 8)),    # no plane 16-byte aligned: dwords
                                             ((560, 576), (0, 16)),                  # padded, 16-byte aligned: the 16-byte path
                                             ((560, 576), (0, 8)),                   # one plane 8-byte aligned only: dwords
                                             ((560, 568), (0, 0)),                   # one pitch off the 16 bytes: dwords
                                             ((552, 552), (0, 0))])                  # tight rows of an odd width: 8-byte aligned rows, dwords
@pytest.mark.parametrize("in_place", [False, True])
def test_pitches_offsets_sentinels_and_inputs(hip_ctx, fixture, pitches, offsets, in_place):
    n, state, exposed = _check_meter(hip_ctx, fixture["scene"], dict(gen.PARAMS), PREVIOUS, pitches=pitches, offsets=offsets, in_place=in_place, work_offset=4)
    assert same(n, fixture["histograms"][0])
    # the metering alone on the same planes, and apply on them
    n2, state2, _ = _check_meter(hip_ctx, fixture["scene"], dict(gen.PARAMS), PREVIOUS, fused=False, pitches=pitches, offsets=offsets)
    assert same(n, n2) and same(state, state2)


# ---- the persistent loop and the ticket -------------------------------------------------------------------------------------------------------
def test_max_workgroups_never_changes_a_byte(hip_ctx):
    w, h = TILES_3X3
    scene_np = ref.random_inputs(w, h, 4242)
    results = [_check_meter(hip_ctx, scene_np, dict(adaptation=0.25, max_workgroups=m), PREVIOUS) for m in (1, 2, 3, 0, 9, 1000)]
    for r in results[1:]:
        assert all(same(a, b) for a, b in zip(results[0], r))


# ---- inputs made to break it --------------------------------------------------------------------------------------------------------------------
def _grey(values):
    img = np.zeros(values.shape + (4,), np.float16)
    img[..., :3] = values[..., None]
    img[..., 3] = 0.5
    return img.view(np.uint16)


def _adversarial():
    w, h = 258, 9
    yy, xx = np.mgrid[0:h, 0:w]
    yield "constant", _grey(np.full((h, w), 0.25)), {}
    yield "two-bin checkerboard", _grey(np.where((xx + yy) % 2 == 0, 0.01, 30.0)), {}
    none = np.zeros((h, w, 4), np.float16)
    for i, v in enumerate((0.0, -0.0, -2.0, np.nan, np.inf, -np.inf)):
        none[:, i::6, 0] = v
    yield "no counted pixel", none.view(np.uint16), {}
    yield "half denormals", _grey(np.random.default_rng(5).integers(1, 1024, (h, w)).astype(np.uint16).view(np.float16)), {}
    yield "beyond both ends", _grey(np.where(xx % 3 == 0, 6e-8, np.where(xx % 3 == 1, 65504.0, 3e-7))), {}
    lognormal = ref.random_inputs(w, h, 77)
    yield "a window of a single pixel", lognormal, dict(low_fraction=0.5, high_fraction=0.5005)
    yield "the whole histogram", lognormal, dict(low_fraction=0.0, high_fraction=1.0)
    yield "an empty window of a metered frame", lognormal, dict(low_fraction=0.5, high_fraction=0.50001)


@pytest.mark.parametrize("case", range(8))
def test_inputs_made_to_break_it(hip_ctx, case):
    name, scene_np, settings = list(_adversarial())[case]
    for state_in, s in ((PREVIOUS, dict(settings, adaptation=0.5)), (None, dict(settings, flags=CUT))):
        n, state, _ = _check_meter(hip_ctx, scene_np, s, state_in, fused=state_in is not None)
        if name == "constant":
            assert (n > 0).sum() == 1 and n.max() == scene_np.shape[0] * scene_np.shape[1]
        if name == "two-bin checkerboard":
            assert (n > 0).sum() == 2
        if name == "no counted pixel":
            assert n.sum() == 0 and state["window"] == 0
            assert state["adapted"] == PREVIOUS["adapted"] if state_in is not None else (state["adapted"].view(np.uint32) == 0x7fc00000 and state["exposure"] == 1)
        if name == "half denormals":
            assert n[0] > 0 and n[1:49].sum() > 0 and n[49:].sum() == 0  # half denormals reach from 2^-24, below bin 1, up to 2^-14
        if name == "beyond both ends":
            assert n[0] > 0 and n[255] > 0
        if name == "a window of a single pixel":
            assert state["window"] == 1
        if name == "the whole histogram":
            assert state["window"] == state["metered"] > 0
        if name == "an empty window of a metered frame":
            assert state["window"] == 0 and state["metered"] > 0


# ---- frames in sequence -------------------------------------------------------------------------------------------------------------------------
def test_four_frames_ping_pong_and_in_place_then_a_cut(hip_ctx):
    import torch
    scenes = [ref.random_inputs(150, 7, 300 + i, median=2.0 ** (3 * i - 4)) for i in range(5)]
    s = dict(adaptation=0.25)
    want, state = [], None
    for i, sc in enumerate(scenes):
        first = i in (0, 4)  # the last frame is a cut
        state = ref.meter(sc, None if first else state, dict(s, flags=CUT if first else 0))[1]
        want.append(state)
    for in_place in (False, True):
        buffers = Buffers()
        at = 0
        for i, sc in enumerate(scenes):
            first = i in (0, 4)
            new = at if in_place else 1 - at
            hip_ctx.exposure_meter(_scene_image(sc).plane, None if first else buffers.state_ptr(at), buffers.state_ptr(new), buffers.work, None,
                                   _params(**dict(s, flags=CUT if first else 0)))
            torch.cuda.synchronize()
            assert same(buffers.state(new), want[i]), f"frame {i}, in place {in_place}: {buffers.state(new)} != {want[i]}"
            at = new
        assert buffers.intact((0,) if in_place else (0, 1))
    assert len({w.tobytes() for w in want}) == 5 and want[4]["adapted"] != want[3]["adapted"]


def test_fused_equals_meter_then_apply_and_row_bands(hip_ctx, fixture):
    import torch
    sc, W, H = fixture["frames"][1], gen.WIDTH, gen.HEIGHT
    p = _params(**gen.PARAMS)
    fused_n, fused_state, fused_out = _check_meter(hip_ctx, sc, dict(gen.PARAMS), PREVIOUS)
    in_place = _check_meter(hip_ctx, sc, dict(gen.PARAMS), PREVIOUS, in_place=True)
    assert all(same(a, b) for a, b in zip((fused_n, fused_state, fused_out), in_place))
    # meter, then apply with state_in
    buffers = Buffers(0, [PREVIOUS, None])
    scene_img, out_img = _scene_image(sc), Image(RGBA16F, W, H, 69 * 8 + 12)
    _meter(hip_ctx, scene_img, buffers, 0, 1, None, p)
    hip_ctx.exposure_apply(scene_img.plane, buffers.state_ptr(0), out_img.plane)
    torch.cuda.synchronize()
    assert same(buffers.histogram(), fused_n) and same(buffers.state(1), fused_state) and same(_texels(out_img), fused_out) and out_img.padding_intact()
    # apply in place
    own = _scene_image(sc, 69 * 8 + 4, 4)
    hip_ctx.exposure_apply(own.plane, buffers.state_ptr(0), own.plane)
    torch.cuda.synchronize()
    assert same(_texels(own), fused_out) and own.padding_intact()
    # row bands write their rows and nothing else, and assemble to the whole
    assembled = np.full((H, W, 4), 0xA5A5, np.uint16)
    for rows in ((9, 10), (0, 9), (10, H), (5, 5), (0, 1), (H - 1, H)):
        band = Image(RGBA16F, W, H, 69 * 8 + 20, None, 8)
        hip_ctx.exposure_apply(scene_img.plane, buffers.state_ptr(0), band.plane, rows)
        torch.cuda.synchronize()
        got = _texels(band)
        assert same(got[rows[0]:rows[1]], fused_out[rows[0]:rows[1]]), f"{rows}: " + differs(got[rows[0]:rows[1]], fused_out[rows[0]:rows[1]])
        assert band.padding_intact(ref.band_rows(rows, H)), f"{rows}: out changed outside the band"
        assert same(got, ref.apply(sc, PREVIOUS["exposure"], rows))
        assembled[rows[0]:rows[1]] = got[rows[0]:rows[1]]
    assert same(assembled, fused_out) and scene_img.unchanged() and buffers.intact((1,))


# ---- the call contract ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip_ctx, fixture):
    """(tests/test_exposure_cpu.py runs the whole list on a context without a device; here: targets, work and states keep their bytes)"""
    import torch
    W, H = gen.WIDTH, gen.HEIGHT
    buffers = Buffers(0, [PREVIOUS, None])
    scene_img, out_img = _scene_image(fixture["scene"]), Image(RGBA16F, W, H)
    sc, out, work, s0, s1 = scene_img.plane, out_img.plane, buffers.work, buffers.state_ptr(0), buffers.state_ptr(1)

    INVALID, FORMAT = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
    ok, nan = _params(), float("nan")
    meter_cases = [((retyped(sc, _abi.FORMAT_R32_SFLOAT), s0, s1, work, out, ok), FORMAT),
                   ((sc, s0, s1, work, retyped(out, _abi.FORMAT_R8G8B8A8_UNORM), ok), FORMAT),
                   ((sc, None, s1, work, out, ok), INVALID),
                   ((sc, s0, None, work, out, ok), INVALID),
                   ((sc, s0, s1, None, out, ok), INVALID),
                   ((sc, None, s1, work, out, _params(flags=CUT)), INVALID),          # the fused form with a cut
                   ((sc, s0, s1, work, out, _params(flags=2)), INVALID),
                   ((sc, s0, s1, work, out, _params(key=0.0)), INVALID),
                   ((sc, s0, s1, work, out, _params(min_exposure=nan)), INVALID),
                   ((sc, s0, s1, work, out, _params(min_exposure=2.0, max_exposure=1.0)), INVALID),
                   ((sc, s0, s1, work, out, _params(low_fraction=0.95, high_fraction=0.5)), INVALID),
                   ((sc, s0, s1, work, out, _params(high_fraction=nan)), INVALID),
                   ((sc, s0, s1, work, out, _params(adaptation=0.0)), INVALID),
                   ((sc, s0, s1, work, out, _params(adaptation=1.5)), INVALID),
                   ((sc, s0, s1 + 2, work, out, ok), INVALID),
                   ((sc, s0, s1, work + 1, out, ok), INVALID),
                   ((sc, s0, s0 + 8, work, out, ok), INVALID),                         # the states half over one another
                   ((sc, s0, work + 512, work, out, ok), INVALID),                     # state_out inside work
                   ((sc, s0, s1, out.ptr + 64, out, ok), INVALID),                     # work inside exposed_out
                   ((sc, s0, sc.ptr + 16, work, out, ok), INVALID),                    # state_out inside the scene
                   ((sc, s0, s1, work, _abi.Plane(out.ptr, W - 1, H, W * 8, RGBA16F), ok), INVALID),
                   ((sc, s0, s1, work, _abi.Plane(sc.ptr + 8, W, H, W * 8, RGBA16F), ok), INVALID)]  # overlapping the scene, not the same plane
    for args, status in meter_cases:
        with pytest.raises(lib.SahError) as e:
            hip_ctx.exposure_meter(*args)
        assert e.value.status == status, args
    apply_cases = [((retyped(sc, _abi.FORMAT_D32_SFLOAT), s0, out), FORMAT), ((sc, s0, retyped(out, _abi.FORMAT_R32_SFLOAT)), FORMAT),
                   ((sc, None, out), INVALID), ((sc, s0, out, (0, H + 1)), INVALID), ((sc, s0, out, (9, 3)), INVALID), ((sc, s0 + 2, out), INVALID),
                   ((sc, out.ptr + 32, out), INVALID), ((sc, s0, _abi.Plane(out.ptr, W, H - 1, W * 8, RGBA16F)), INVALID),
                   ((sc, s0, _abi.Plane(sc.ptr + W * 8, W, H, W * 8, RGBA16F)), INVALID)]
    for args, status in apply_cases:
        with pytest.raises(lib.SahError) as e:
            hip_ctx.exposure_apply(*args)
        assert e.value.status == status, args
    torch.cuda.synchronize()
    assert out_img.unchanged() and scene_img.unchanged() and buffers.unchanged()


def test_side_stream_captured_graph_replayed_twice_and_no_side_effects(fixture):
    import torch
    with side_stream_context() as (ctx, s):
        W, H = gen.WIDTH, gen.HEIGHT
        settings = dict(gen.PARAMS)
        params = _params(**settings)
        buffers = Buffers(0, [PREVIOUS, None])
        scene_img, out_img = _scene_image(fixture["scene"]), Image(RGBA16F, W, H)
        state = context_state(ctx)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.exposure_meter(scene_img.plane, buffers.state_ptr(0), buffers.state_ptr(1), buffers.work, out_img.plane, params)
        s.synchronize()
        assert same(buffers.histogram(), fixture["histograms"][0]) and same(buffers.state(1), ref.meter(fixture["scene"], PREVIOUS, settings)[1])
        assert context_state(ctx) == state
        # one captured graph (the kernel that zeroes work, then the metering kernel: a linear chain), replayed twice over other scene contents
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.exposure_meter(scene_img.plane, buffers.state_ptr(0), buffers.state_ptr(1), buffers.work, out_img.plane, params)
        for seed in (77, 78):
            other = ref.random_inputs(W, H, seed, median=0.1 * (seed - 70))
            scene_img.t.copy_(_scene_image(other).t)
            out_img.t.fill_(SENTINEL)
            buffers.t[buffers.work_at:buffers.work_at + 1040].fill_(SENTINEL)  # (the replay zeroes it first)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            want_n, want_state = ref.meter(other, PREVIOUS, settings)
            assert same(buffers.histogram(), want_n), f"replay with seed {seed}: " + differs(buffers.histogram(), want_n)
            assert same(buffers.state(1), want_state) and same(_texels(out_img), ref.apply(other, PREVIOUS["exposure"]))
        assert context_state(ctx) == state


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------------
EXTENTS = [(80, 36), (80, 36), (45, 50)]


def _wrapper_frames(seed):
    return [ref.random_inputs(w, h, seed + i, median=2.0 ** (2 * i - 3)) for i, (w, h) in enumerate(EXTENTS)]


def _wrapper_sequence(frames, adaptation):
    """what either wrapper gives: the third frame has another extent, so it has no history again"""
    first = gen.sequence(frames[:2], dict(adaptation=adaptation))
    return first + gen.sequence(frames[2:], dict(adaptation=adaptation))


def test_three_frames_through_the_python_wrapper(hip_ctx):
    import torch
    frames = _wrapper_frames(900)
    auto = frame.AutoExposure(hip_ctx, *EXTENTS[0], adaptation=0.25)
    assert auto.params.key == f32(0.18) and auto.params.low_fraction == 0.5 and auto.params.max_exposure == 64.0  # the header's defaults unless changed
    for i, (sc, (want_n, want_state, want_exposed)) in enumerate(zip(frames, _wrapper_sequence(frames, 0.25))):
        out = auto.expose(util.to_torch(sc))
        torch.cuda.synchronize()
        assert out is auto.exposed and tuple(out.shape) == sc.shape
        assert same(auto.histogram(), want_n) and same(bytes(auto.state()), want_state), f"frame {i}"
        got = out.cpu().numpy().view(np.uint16)
        assert same(got, want_exposed), f"frame {i}: " + differs(got, want_exposed)
    auto.reset()
    out = auto.expose(util.to_torch(frames[2]))  # after a cut: metered, then exposed by its own state
    torch.cuda.synchronize()
    assert same(out.cpu().numpy().view(np.uint16), want_exposed) and same(bytes(auto.state()), want_state)


def test_three_frames_through_the_cpp_facade(tmp_path):
    frames = _wrapper_frames(950)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(frames)], np.uint32).tobytes() + f32(0.25).tobytes())
        for sc in frames:
            f.write(np.array([sc.shape[1], sc.shape[0]], np.uint32).tobytes() + sc.tobytes())
    subprocess.check_call([host_program("host_exposure", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    at = 0
    for i, (sc, (want_n, want_state, want_exposed)) in enumerate(zip(frames, _wrapper_sequence(frames, 0.25))):
        state, n = blob[at:at + 16], np.frombuffer(blob[at + 16:at + 16 + 1024], np.uint32)
        exposed = np.frombuffer(blob[at + 1040:at + 1040 + sc.nbytes], np.uint16).reshape(sc.shape)
        at += 1040 + sc.nbytes
        assert same(n, want_n) and state == want_state.tobytes(), f"frame {i}: {np.frombuffer(state, ref.STATE)} != {want_state}"
        assert same(exposed, want_exposed), f"frame {i}: " + differs(exposed, want_exposed)
    assert at == len(blob)


# ---- the frame the pass exists for -------------------------------------------------------------------------------------------------------------
def test_atrium_lit_with_the_sun_eight_times_brighter_is_exposed_alike(hip_ctx):
    """sah_gbuffer_render of the atrium at 128 x 72 and sah_lighting in LPV mode, once as it is and once with the sun's colour multiplied by
    8; AutoExposure with adaptation 1 on both (its clamp opened to 2^+-12: with the default 1/64 the bright frame's exposure, 0.0069, would
    be clamped); then sah_bloom and sah_tonemap.

    The bounds come from the restatement alone: re-metering an image exposed by its own state lands within a bin's width of the key —
    2^0.09 at most over 200 random log-normal 69 x 21 images with scale changes of 8, 1/8 and 3 in a numpy prototype, 2^0.062 over the
    cases of tests/test_exposure_cpu.py, and on this scene, lit by the CPU oracle, 2^0.001 and 2^0.024 — so 2^0.25 holds with room.
    The sun-blend quirk of the lighting pass makes the sunlit pixels of the bright frame 63 times brighter, not 8 (the oracle's figures:
    the metered averages differ by 2^4.19), so the unexposed planes are asserted to differ by MORE than 8 in the metered average.  The
    oracle's composite of the unexposed bright frame has 87 % of its pixels at code 250 or above in all channels, the exposed one 7 %."""
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
    settings = dict(min_exposure=2.0 ** -12, max_exposure=2.0 ** 12)
    cut = dict(settings, flags=CUT)
    lit, exposed, states, composites = {}, {}, {}, {}
    for gain in (1, 8):
        f = util.LightingFrame(W, H, gbuffer=gb_np, seed=3, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV)
        for c in range(3):
            f.sun.constants.color[c] *= gain
        lit[gain] = f.run_hip(hip_ctx)
        auto = frame.AutoExposure(hip_ctx, W, H, **settings)
        lit_t = util.to_torch(lit[gain])
        out = auto.expose(lit_t)
        torch.cuda.synchronize()
        exposed[gain], states[gain] = out.cpu().numpy().view(np.uint16), np.frombuffer(bytes(auto.state()), ref.STATE)[0]
        want_n, want_state = ref.meter(lit[gain], None, cut)
        assert same(auto.histogram(), want_n) and same(states[gain], want_state) and same(exposed[gain], ref.apply(lit[gain], want_state["exposure"]))
        for name, plane_t in (("unexposed", lit_t), ("exposed", out)):
            mips = [torch.zeros((mh, mw, 4), dtype=torch.int16, device="cuda") for (mw, mh) in images.bloom_mip_sizes(W, H, 6)]
            ldr = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
            p, chain = images.plane(plane_t, RGBA16F), images.mipchain(mips)
            hip_ctx.bloom(p, chain)
            hip_ctx.tonemap(p, chain, images.plane(ldr, _abi.FORMAT_R8G8B8A8_SRGB))
            torch.cuda.synchronize()
            composites[gain, name] = ldr.cpu().numpy()[..., :3]
    remetered = {}
    for gain in (1, 8):
        st = states[gain]
        l_avg = float(ref.l_avg_of(st["adapted"]))
        assert st["window"] > 1000 and 2.0 ** -12 < st["exposure"] < 2.0 ** 12  # metered, not clamped
        assert abs(float(st["exposure"]) * l_avg / 0.18 - 1) < 1e-6  # exposure x the frame's own L_avg is the key
        remetered[gain] = float(ref.meter(exposed[gain], None, cut)[1]["exposure"])
        print(f"sun x {gain}: exposure {float(st['exposure']):.5f}, adapted {float(st['adapted']):.4f}, re-metered exposure 2^{np.log2(remetered[gain]):+.4f}")
        assert abs(np.log2(remetered[gain])) < 0.25
    assert abs(np.log2(remetered[8] / remetered[1])) < 0.25
    octaves = float(states[8]["adapted"]) - float(states[1]["adapted"])
    print(f"the unexposed frames' metered averages differ by 2^{octaves:.3f}")
    assert octaves > 3.0  # more than 8 times (see above)
    saturated = {k: (v >= 250).all(-1) for k, v in composites.items()}
    print("saturated: " + ", ".join(f"sun x {g} {n} {float(saturated[g, n].mean()):.3f}" for g, n in sorted(saturated)))
    assert saturated[8, "unexposed"].mean() > 0.5
    assert (saturated[8, "exposed"] & saturated[8, "unexposed"]).sum() < 0.25 * saturated[8, "unexposed"].sum()
    assert saturated[1, "exposed"].mean() < 0.05 and 40 < composites[8, "exposed"].mean() < 215 and 40 < composites[1, "exposed"].mean() < 215
