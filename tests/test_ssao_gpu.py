"""GPU: sah_ssao (include/sah_ssao.h) against the numpy restatement (tests/ssao_ref.py) run on the device's own planes, and its committed
fixture, bit for bit; the Python ScreenSpaceAO and the C++ façade's AmbientOcclusionPhase over successive frames; and the frame the pass
exists for — the rasterised atrium, its AO, and the LPV-mode lighting on that AO plane.  The raw kernel's tile is 64 x 16 pixels, the blur
kernel's 32 x 16."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, lib, mesh, scene
from tests import ssao_ref as ref
from tests import util
from tests.host_programs import host_program
from tests.support import context_state, differs, Image, retyped, same, SENTINEL, side_stream_context, view_data_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_ssao as gen  # noqa: E402

f32 = np.float32
D32, RGBA16F, R32F = _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R32_SFLOAT
SENTINEL_F32 = np.frombuffer(bytes([SENTINEL] * 4), f32)[0]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)  # each test under a limit of its own: an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fixture():
    fx = np.load(gen.FIXTURE)
    return {"depth": np.ascontiguousarray(fx["depth_plane"][:, :gen.WIDTH]), "normals": np.ascontiguousarray(fx["normals_plane"][:, :gen.WIDTH]),
            "ao": [fx[f"ao_blur{b}"] for b in (0, 1, 2)]}


def scene_view(w, h, jitter=(0.3, -0.2)):
    v = scene.SceneView.default(w, h)
    v.jitter = np.array(jitter, f32)
    v.update_transforms()
    return v.gpu_data


def _params(**changes):
    return _abi.SsaoParams.default(**changes)


class Planes:
    """the four device planes of one call; pitches / offsets in the order depth, normals, scratch, ao_out"""

    def __init__(self, depth, normals, pitches=(None,) * 4, offsets=(0,) * 4):
        h, w = depth.shape
        self.w, self.h = w, h
        self.depth = Image(D32, w, h, pitches[0], depth, offsets[0])
        self.normals = Image(RGBA16F, w, h, pitches[1], normals, offsets[1])
        self.scratch = Image(R32F, w, h, pitches[2], None, offsets[2])
        self.out = Image(R32F, w, h, pitches[3], None, offsets[3])

    def run(self, ctx, view_data, params, rows=(0, 0), scratch=True):
        import torch
        ctx.ssao(view_data, self.depth.plane, self.normals.plane, self.scratch.plane if scratch else None, self.out.plane, params, rows)
        torch.cuda.synchronize()
        assert self.depth.unchanged() and self.normals.unchanged()
        return self.out.texels(f32).reshape(self.h, self.w)


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 2])
def test_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture, passes):
    view, params = view_data_of(gen.view()), _params(**dict(gen.PARAMS, blur_passes=passes))
    p = Planes(fixture["depth"], fixture["normals"])
    got = p.run(hip_ctx, view, params)
    assert same(got, fixture["ao"][passes]), differs(got, fixture["ao"][passes])
    if passes:
        assert same(p.scratch.texels(f32).reshape(p.h, p.w), fixture["ao"][0])  # the scratch plane is the raw result
    else:
        assert p.scratch.unchanged() and same(Planes(fixture["depth"], fixture["normals"]).run(hip_ctx, view, params, scratch=False), got)
    again = Planes(fixture["depth"], fixture["normals"]).run(hip_ctx, view, params)
    assert same(again, got)


# ---- extents --------------------------------------------------------------------------------------------------------------------------------
# raw tile 64 x 16, blur tile 32 x 16: one below, at and one above each in each dimension; (192, 48): three raw tiles by three
@pytest.mark.parametrize("extent", [(1, 1), (2, 3), (63, 15), (64, 16), (65, 17), (31, 16), (32, 17), (33, 15), (192, 48)])
@pytest.mark.parametrize("passes", [0, 2])
def test_extents_and_radius_caps(hip_ctx, extent, passes):
    w, h = extent
    depth, normals = ref.random_inputs(w, h, 7 * w + h)
    view = scene_view(w, h)
    p = Planes(depth, normals)
    darkened = 0
    for cap in (1.0, 2.0, 32.0, 2.0 * max(w, h) + 50.0):  # the last: larger than the image
        settings = dict(radius=1.5, max_radius_pixels=cap, blur_passes=passes, fade_out_from=3.0, fade_out_to=9.0)
        got = p.run(hip_ctx, view, _params(**settings))
        want, info = ref.ssao_ex(depth, normals, ref.View(view), settings)
        assert same(got, want), f"max_radius_pixels {cap}: " + differs(got, want)
        darkened += int((want < 1).sum())
        if w * h >= 64 and cap > 2:
            assert (info["r_px"][info["live"]] > 2).any()
    if w * h >= 64:
        assert darkened > w * h and (~np.isfinite(depth)).any() and (depth == 0).any()  # (not because everything is 1.0; sky and NaN are there)


# ---- pitches and alignment ----------------------------------------------------------------------------------------------------------------
# pitches and offsets in bytes: depth, normals, scratch, ao_out
@pytest.mark.parametrize("pitches,offsets", [((69 * 4 + 12, 69 * 8 + 4, 69 * 4 + 20, 69 * 4 + 4), (4, 8, 12, 4)),   # no plane 16-byte aligned: dwords
                                             ((288, 560, 304, 288), (0, 16, 32, 0)),                               # padded, 16-byte aligned: the 16-byte path
                                             ((288, 560, 304, 288), (0, 8, 0, 0)),                                 # one input 8-byte aligned only: dwords
                                             ((288, 560, 292, 288), (0, 0, 0, 0))])                                # the raw pass's target off the 16-byte pitch
@pytest.mark.parametrize("passes", [0, 2])
def test_pitches_offsets_sentinels_and_inputs(hip_ctx, fixture, pitches, offsets, passes):
    p = Planes(fixture["depth"], fixture["normals"], pitches, offsets)
    got = p.run(hip_ctx, view_data_of(gen.view()), _params(**dict(gen.PARAMS, blur_passes=passes)))  # (asserts the inputs unchanged)
    assert same(got, fixture["ao"][passes]), differs(got, fixture["ao"][passes])
    assert p.out.padding_intact() and p.scratch.padding_intact()
    assert p.scratch.unchanged() if passes == 0 else same(p.scratch.texels(f32).reshape(p.h, p.w), fixture["ao"][0])


# ---- row bands --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 2])
def test_row_bands_write_their_rows_and_nothing_else(hip_ctx, fixture, passes):
    W, H = gen.WIDTH, gen.HEIGHT
    view, params = view_data_of(gen.view()), _params(**dict(gen.PARAMS, blur_passes=passes))
    whole = fixture["ao"][passes]
    assembled = np.full((H, W), np.nan, f32)
    for rows in ((9, 10), (0, 9), (10, H), (17, 19), (5, 5), (0, 0 + 1), (H - 1, H)):
        p = Planes(fixture["depth"], fixture["normals"], (None, None, 69 * 4 + 12, 69 * 4 + 28))
        got = p.run(hip_ctx, view, params, rows)
        assert same(got[rows[0]:rows[1]], whole[rows[0]:rows[1]]), f"{rows}: " + differs(got[rows[0]:rows[1]], whole[rows[0]:rows[1]])
        assert p.out.padding_intact(rows), f"{rows}: ao_out changed outside the band"
        raw_rows = ref.band_rows(rows, H, passes) if passes else (0, 0)  # the rows of scratch the header names
        assert p.scratch.padding_intact(raw_rows), f"{rows}: scratch changed outside rows {raw_rows}"
        assert same(p.scratch.texels(f32).reshape(H, W)[raw_rows[0]:raw_rows[1]], fixture["ao"][0][raw_rows[0]:raw_rows[1]])
        assembled[rows[0]:rows[1]] = got[rows[0]:rows[1]]
    assert same(assembled, whole)


# ---- the call contract ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip_ctx, fixture):
    """(tests/test_ssao_cpu.py runs the whole list on a context without a device; here: the targets keep their bytes)"""
    import torch
    p = Planes(fixture["depth"], fixture["normals"])
    view, ok = view_data_of(gen.view()), _params(**gen.PARAMS)
    depth, normals, scratch, out = p.depth.plane, p.normals.plane, p.scratch.plane, p.out.plane

    bad_view = view_data_of(gen.view())
    bad_view.z_near = float("nan")
    INVALID, FORMAT = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
    P = lambda **kw: _params(**dict(gen.PARAMS, **kw))  # noqa: E731
    cases = [((view, depth, normals, scratch, retyped(out, D32), ok), FORMAT),
             ((view, retyped(depth, R32F), normals, scratch, out, ok), FORMAT),
             ((view, depth, normals, retyped(scratch, D32), out, ok), FORMAT),
             ((view, depth, normals, None, out, ok), INVALID),
             ((view, depth, normals, scratch, out, ok, (0, 22)), INVALID),
             ((view, depth, normals, scratch, out, ok, (9, 3)), INVALID),
             ((view, depth, normals, scratch, out, P(flags=1)), INVALID),
             ((view, depth, normals, scratch, out, P(blur_passes=3)), INVALID),
             ((view, depth, normals, scratch, out, P(radius=0.0)), INVALID),
             ((view, depth, normals, scratch, out, P(radius=float("inf"))), INVALID),
             ((view, depth, normals, scratch, out, P(max_radius_pixels=0.5)), INVALID),
             ((view, depth, normals, scratch, out, P(shadow_clamp=1.5)), INVALID),
             ((view, depth, normals, scratch, out, P(horizon_angle_threshold=-0.1)), INVALID),
             ((view, depth, normals, scratch, out, P(fade_out_from=30.0)), INVALID),
             ((view, depth, normals, scratch, out, P(edge_sharpness=float("nan"))), INVALID),
             ((bad_view, depth, normals, scratch, out, ok), INVALID),
             ((view, depth, normals, out, out, ok), INVALID),
             ((view, depth, normals, scratch, scratch, ok), INVALID),
             ((view, depth, normals, scratch, _abi.Plane(out.ptr, 68, 21, 69 * 4, R32F), ok), INVALID)]
    for args, status in cases:
        with pytest.raises(lib.SahError) as e:
            hip_ctx.ssao(*args)
        assert e.value.status == status, args
    torch.cuda.synchronize()
    assert p.out.unchanged() and p.scratch.unchanged() and p.depth.unchanged() and p.normals.unchanged()


def test_side_stream_captured_graph_replayed_twice_and_no_side_effects(fixture):
    import torch
    with side_stream_context() as (ctx, s):
        W, H = gen.WIDTH, gen.HEIGHT
        view, params = view_data_of(gen.view()), _params(**dict(gen.PARAMS, blur_passes=2))
        a = Planes(fixture["depth"], fixture["normals"])
        state = context_state(ctx)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.ssao(view, a.depth.plane, a.normals.plane, a.scratch.plane, a.out.plane, params)
        s.synchronize()
        assert same(a.out.texels(f32).reshape(H, W), fixture["ao"][2])
        assert context_state(ctx) == state
        # one captured graph (raw, then blur: a linear chain), replayed twice over other input contents
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.ssao(view, a.depth.plane, a.normals.plane, a.scratch.plane, a.out.plane, params)
        for seed in (77, 78):
            depth, normals = ref.random_inputs(W, H, seed)
            b = Planes(depth, normals)
            a.depth.t.copy_(b.depth.t)
            a.normals.t.copy_(b.normals.t)
            a.out.t.fill_(SENTINEL)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            want = ref.ssao(depth, normals, gen.view(), dict(gen.PARAMS, blur_passes=2))
            got = a.out.texels(f32).reshape(H, W)
            assert same(got, want), f"replay with seed {seed}: " + differs(got, want)
            assert (want < 1).sum() > 200


# ---- the frame the pass exists for -------------------------------------------------------------------------------------------------------------
def test_atrium_rasterised_then_ssao_then_lpv_lighting(hip_ctx):
    """sah_gbuffer_render of the atrium at 128 x 72, sah_ssao on its depth and normals (equal to the restatement on the device's planes),
    sah_lighting in LPV mode on that AO plane (equal to the oracle lighting on the same plane): a frame with a real AO plane and no
    acceleration structure."""
    import torch
    W, H = 128, 72
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    view = scene.SceneView.default(W, H)
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    gb = {k: torch.zeros((H, W) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
    frame.rasterised_frame(hip_ctx, geo, view.gpu_data, gb)
    ssao = frame.ScreenSpaceAO(hip_ctx, W, H, radius=2.0)
    ao_t = ssao.generate(view.gpu_data, gb["depth"], gb["normals"])
    torch.cuda.synchronize()
    gb_np = {k: v.cpu().numpy() for k, v in gb.items()}
    gb_np["normals"] = gb_np["normals"].view(np.uint16)
    ao = ao_t.cpu().numpy()
    want, info = ref.ssao_ex(gb_np["depth"], gb_np["normals"], ref.View(view.gpu_data), dict(radius=2.0))
    assert same(ao, want), differs(ao, want)
    covered = gb_np["depth"] > 0
    print(f"atrium {W} x {H}: {float(covered.mean()):.2f} covered, AO below 1 at {float((ao < 1).mean()):.2f} of the pixels, minimum {float(ao.min()):.3f}, "
          f"mean {float(ao[covered].mean()):.3f}")
    assert covered.mean() > 0.5 and 0.1 < (ao[covered] < 1).mean() and ao[covered].mean() > 0.5 and (ao[~covered] == 1).all()
    f = util.LightingFrame(W, H, gbuffer=gb_np, seed=3, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV)
    assert bytes(f.view.gpu_data) == bytes(view.gpu_data)
    flat = f.run_hip(hip_ctx)  # the synthetic AO plane the frame had before: the AO plane matters to the result
    f.arrays["ao"] = ao
    got, oracle = f.run_hip(hip_ctx), f.run_oracle()
    d = util.f16_ulp_diff(got, oracle)
    print(util.report_ulp("atrium, LPV lighting on the SSAO plane", d))
    assert d.max() == 0 and (got != flat).any()


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------------
def _frames(extents, seed):
    return [(w, h, (0.25 * i - 0.375, 0.125 * i + 0.125), *ref.random_inputs(w, h, seed + i)) for i, (w, h) in enumerate(extents)]  # dyadic jitters, never 0


def test_three_frames_through_the_python_wrapper(hip_ctx):
    import torch
    W, H = 96, 40
    ssao = frame.ScreenSpaceAO(hip_ctx, W, H, radius=1.5, fade_out_from=3.0, fade_out_to=9.0)
    assert ssao.params.blur_passes == 2 and ssao.params.max_radius_pixels == 32.0  # the reference's CACAO settings unless changed
    for w, h, jitter, depth, normals in _frames([(W, H)] * 3, 900):
        view = scene_view(w, h, jitter)
        out = ssao.generate(view, torch.from_numpy(depth).cuda(), util.to_torch(normals))
        torch.cuda.synchronize()
        assert out is ssao.ao
        want = ref.ssao(depth, normals, ref.View(view), dict(radius=1.5, fade_out_from=3.0, fade_out_to=9.0))
        assert same(out.cpu().numpy(), want), differs(out.cpu().numpy(), want)
        assert (want < 1).mean() > 0.2
    unblurred = frame.ScreenSpaceAO(hip_ctx, W, H, radius=1.5, blur_passes=0, fade_out_from=3.0, fade_out_to=9.0)
    out = unblurred.generate(view, torch.from_numpy(depth).cuda(), util.to_torch(normals))
    torch.cuda.synchronize()
    assert same(out.cpu().numpy(), ref.ssao(depth, normals, ref.View(view), dict(radius=1.5, blur_passes=0, fade_out_from=3.0, fade_out_to=9.0)))
    assert (unblurred.scratch == 1).all()  # not touched


@pytest.mark.parametrize("passes", [2, 0])
def test_three_frames_through_the_cpp_facade(tmp_path, hip_ctx, passes):
    """AmbientOcclusionPhase with AoTechnique::ScreenSpace: the façade's own SceneView forms the view block, which comes back with each AO
    plane; the third frame has another extent, so the phase re-creates its scratch texture."""
    radius = 1.5
    frames = _frames([(80, 36), (80, 36), (45, 50)], 950)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(frames), passes], np.uint32).tobytes() + f32(radius).tobytes())
        for w, h, jitter, depth, normals in frames:
            f.write(np.array([w, h], np.uint32).tobytes() + np.array(jitter, f32).tobytes() + depth.tobytes() + normals.tobytes())
    subprocess.check_call([host_program("host_ssao", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    at = 0
    for i, (w, h, jitter, depth, normals) in enumerate(frames):
        view = _abi.ViewData.from_buffer_copy(blob[at:at + 432])
        facade = np.frombuffer(blob[at + 432:at + 432 + w * h * 4], f32).reshape(h, w)
        at += 432 + w * h * 4
        assert tuple(view.render_resolution) == (w, h) and tuple(view.jitter) == tuple(f32(j) for j in jitter) and view.projection[8] != 0 and view.projection[9] != 0
        settings = dict(radius=radius, blur_passes=passes)  # everything else: the reference's CACAO settings
        want = ref.ssao(depth, normals, ref.View(view), settings)
        assert same(facade, want), f"frame {i}: " + differs(facade, want)
        got = Planes(depth, normals).run(hip_ctx, view, _params(**settings))
        assert same(facade, got) and (want < 1).mean() > 0.1
    assert at == len(blob)
