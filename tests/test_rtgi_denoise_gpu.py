"""GPU: sah_rtgi_denoise (include/sah_rtgi_denoise.h) against the numpy restatement (tests/rtgi_denoise_ref.py) run on the device's own
planes, and its committed fixture, bit for bit in all four outputs; the call's contract (row bands, refusals, NULL previous planes, a
captured graph); frame.RtgiDenoiser and the C++ façade over successive frames; and the frame the pass exists for.  The temporal kernel's
tile is 64 x 8 pixels, the filter kernel's 16 x 16."""
import faulthandler
import os
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, lib, scene
from tests import rtgi_denoise_ref as ref
from tests import util
from tests.host_programs import host_program
from tests.support import context_state, differs, Image, reprojection_view_data_of, retyped, same, SENTINEL, side_stream_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_rtgi_denoise as gen  # noqa: E402

f32 = np.float32
D32, RGBA16F, RG16F, RGBA32F, RG32F = (_abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R16G16_SFLOAT,
                                      _abi.FORMAT_R32G32B32A32_SFLOAT, _abi.FORMAT_R32G32_SFLOAT)
INPUTS = (("ray_buffer", RGBA16F), ("ray_irradiance", RGBA16F), ("depth", D32), ("normals", RGBA16F), ("motion_vectors", RG16F), ("previous_depth", D32),
          ("history", RGBA32F), ("history_moments", RG32F))
OUTPUTS = (("accum_out", RGBA32F), ("moments_out", RG32F), ("denoised_ray_buffer", RGBA16F), ("denoised_irradiance", RGBA16F))
OUT_SHAPE = {"accum_out": (f32, 4), "moments_out": (f32, 2), "denoised_ray_buffer": (np.uint16, 4), "denoised_irradiance": (np.uint16, 4)}
NAMES = [n for n, _ in INPUTS + OUTPUTS]
ORDER = [n for n, _ in INPUTS]
PREVIOUS = ("previous_depth", "history", "history_moments")


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)  # each test under a limit of its own: an overrun ends the process
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(gen.FIXTURE))


def moved_view(w, h, dolly=0.05, jitter=(0.3, -0.2)):
    """a SceneView's block whose last_frame_view stands `dolly` further back along the view axis"""
    v = scene.SceneView.default(w, h)
    v.jitter = np.array(jitter, f32)
    v.update_transforms()
    d = _abi.ViewData.from_buffer_copy(bytes(v.gpu_data))
    for i in range(16):
        d.last_frame_view[i] = d.view[i]
    d.last_frame_view[14] = d.view[14] - dolly
    return d


def _params(**changes):
    return _abi.RtgiDenoiseParams.default(**changes)


def pitch_of(fmt, w):
    return w * _abi.FORMAT_BPP[fmt]  # every texel here is a multiple of 4 bytes: the smallest pitch the argument check admits


class Planes:
    """the twelve device planes of one call; `layout`: {name: (pitch, offset)} in bytes; `inputs`: the eight input planes by name (None:
    the plane is not created and NULL is passed)"""

    def __init__(self, inputs, layout=None):
        h, w = inputs["depth"].shape
        self.w, self.h, self.images = w, h, {}
        layout = layout or {}
        for name, fmt in INPUTS + OUTPUTS:
            data = inputs.get(name)
            if name in dict(INPUTS) and data is None:
                continue
            pitch, offset = layout.get(name, (pitch_of(fmt, w), 0))
            self.images[name] = Image(fmt, w, h, pitch, data, offset)

    def desc(self, **replaced):
        planes = {n: im.plane for n, im in self.images.items()}
        planes.update(replaced)
        return _abi.RtgiDenoiseDesc.of(**planes)

    def run(self, ctx, view_data, params, rows=(0, 0)):
        import torch
        ctx.rtgi_denoise(view_data, self.desc(), params, rows)
        torch.cuda.synchronize()
        assert all(self.images[n].unchanged() for n, _ in INPUTS if n in self.images)
        return self.outputs()

    def outputs(self):
        return tuple(self.images[n].texels(OUT_SHAPE[n][0]).reshape(self.h, self.w, OUT_SHAPE[n][1]) for n, _ in OUTPUTS)


def assert_outputs(got, want, what=""):
    for (name, _), g, w in zip(OUTPUTS, got, want):
        assert same(g, w), f"{what} {name}: " + differs(g, w)


def reference(inputs, view, settings):
    return ref.denoise(*[inputs.get(k) for k in ORDER], view, settings)


def fixture_want(fx, i, passes):
    """the four outputs of frame i: the denoised ray buffer is stored for frame 0; it is the unit normal and the input's distance, which
    the restatement gives for the others"""
    inputs = gen.frame_of(fx, i)
    ok, _, _, N, _ = ref.surfaces(inputs["depth"], inputs["normals"], gen.view(i))
    drb = ref.pack(inputs["ray_buffer"], inputs["ray_irradiance"], ok, N, np.zeros(ok.shape + (3,), f32))[0]
    if i == 0:
        assert same(drb, fx["denoised_ray_buffer0"])
    return fx[f"accum{i}"], fx[f"moments{i}"], drb, fx[f"denoised_irradiance{i}_passes{passes}"]


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 2, 3])
def test_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture, passes):
    for i in range(gen.FRAMES):
        inputs, view, params = gen.frame_of(fixture, i), reprojection_view_data_of(gen.view(i)), _params(**gen.params(i, passes))
        got = Planes(inputs).run(hip_ctx, view, params)
        assert_outputs(got, fixture_want(fixture, i, passes), f"frame {i}")
        assert_outputs(Planes(inputs).run(hip_ctx, view, params), got, f"frame {i} again")


# ---- extents --------------------------------------------------------------------------------------------------------------------------------
# temporal tile 64 x 8, filter tile 16 x 16: one below, at and one above each in each axis; an odd extent of three temporal tiles by five
@pytest.mark.parametrize("extent", [(1, 1), (3, 2), (63, 7), (64, 8), (65, 9), (15, 15), (16, 16), (17, 17), (131, 37)])
@pytest.mark.parametrize("passes", [0, 1, 2, 3])
def test_extents(hip_ctx, extent, passes):
    w, h = extent
    inputs = ref.random_inputs(w, h, 7 * w + h)
    view = moved_view(w, h)
    settings = dict(passes=passes, jitter=(0.25, -0.125), previous_jitter=(-0.25, 0.375), max_history=24.0)
    got = Planes(inputs).run(hip_ctx, view, _params(**settings))
    accum, moments, drb, dirr, info = ref.denoise_ex(*[inputs[k] for k in ORDER], ref.View(view), settings)
    assert_outputs(got, (accum, moments, drb, dirr), f"{w} x {h}")
    if w * h >= 64:  # (not because nothing happens)
        assert info["history"].sum() > w * h // 8 and info["depth_rejected"].any() and (info["taps_valid"] > 1).any() and (~info["ok"]).any()
        assert info["short"].any() and (info["ok"] & ~info["short"]).any()
        if passes:
            assert info["filter"][0]["luminance_active"].any() and (info["planes"][-1] != info["planes"][0]).any(-1).sum() > w * h // 4


# ---- pitches and alignment ----------------------------------------------------------------------------------------------------------------
def _layout(pad, offset):
    """every plane with `pad` bytes more than a row and a base shifted by `offset`"""
    return {n: (pitch_of(f, gen.WIDTH) + pad, offset) for n, f in INPUTS + OUTPUTS}


_ALIGNED = {n: ((pitch_of(f, gen.WIDTH) + 31) // 16 * 16, 0) for n, f in INPUTS + OUTPUTS}
LAYOUTS = {"dwords: nothing 16-byte aligned": _layout(4, 4),
           "16-byte path: padded, shifted by 32": {n: (p, 32) for n, (p, _) in _ALIGNED.items()},
           "one input 8-byte aligned only": dict(_ALIGNED, ray_irradiance=(_ALIGNED["ray_irradiance"][0], 8)),
           "moments_out off the 16-byte pitch": dict(_ALIGNED, moments_out=(pitch_of(RG32F, gen.WIDTH) + 4, 0))}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("passes", [0, 3])
def test_pitches_offsets_sentinels_and_inputs(hip_ctx, fixture, layout, passes):
    for i in (0, 1):
        p = Planes(gen.frame_of(fixture, i), LAYOUTS[layout])
        got = p.run(hip_ctx, reprojection_view_data_of(gen.view(i)), _params(**gen.params(i, passes)))  # (asserts the inputs unchanged)
        assert_outputs(got, fixture_want(fixture, i, passes), f"frame {i}")
        assert all(p.images[n].padding_intact() for n, _ in OUTPUTS)


# ---- row bands --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 3])
def test_row_bands_write_their_rows_and_nothing_else(hip_ctx, fixture, passes):
    W, H = gen.WIDTH, gen.HEIGHT
    view, params = reprojection_view_data_of(gen.view(1)), _params(**gen.params(1, passes))
    whole = fixture_want(fixture, 1, passes)
    assembled = [np.full((H, W, c * np.dtype(t).itemsize), SENTINEL, np.uint8).view(t) for t, c in (OUT_SHAPE[n] for n, _ in OUTPUTS)]
    for rows in ((9, 10), (0, 9), (10, H), (17, 19), (5, 5), (0, 1), (H - 1, H)):
        p = Planes(gen.frame_of(fixture, 1), _layout(12, 0))
        got = p.run(hip_ctx, view, params, rows)
        wide = ref.band_rows(rows, H, passes)
        for k, (name, _) in enumerate(OUTPUTS):
            r = rows if name.startswith("denoised") else wide
            assert same(got[k][r[0]:r[1]], whole[k][r[0]:r[1]]), f"{rows} {name}: " + differs(got[k][r[0]:r[1]], whole[k][r[0]:r[1]])
            assert p.images[name].padding_intact(r), f"{rows}: {name} changed outside rows {r}"
            assembled[k][r[0]:r[1]] = got[k][r[0]:r[1]]
    assert_outputs(assembled, whole, "assembled")


# ---- the call contract ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip_ctx, fixture):
    import torch
    p = Planes(gen.frame_of(fixture, 1))
    view, ok = reprojection_view_data_of(gen.view(1)), _params(**gen.params(1, 3))
    pl = {n: im.plane for n, im in p.images.items()}

    def shaped(name, **kw):
        q = _abi.Plane(pl[name].ptr, pl[name].width, pl[name].height, pl[name].row_pitch_bytes, pl[name].format)
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    bad_view = reprojection_view_data_of(gen.view(1))
    bad_view.z_near = float("nan")
    nan_view = reprojection_view_data_of(gen.view(1))
    nan_view.last_frame_view[10] = float("nan")
    zero_view = reprojection_view_data_of(gen.view(1))
    zero_view.z_near = 0.0
    INVALID, FORMAT = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
    P = lambda **kw: _params(**dict(gen.params(1, 3), **kw))  # noqa: E731
    inf, nan = float("inf"), float("nan")
    cases = [((view, p.desc(**{n: retyped(pl[n], D32 if f != D32 else _abi.FORMAT_R32_SFLOAT)}), ok), FORMAT) for n, f in INPUTS + OUTPUTS]
    cases += [((view, p.desc(**{n: None}), ok), INVALID) for n in NAMES]  # a previous-frame plane may be NULL only with the flag
    cases += [((view, p.desc(), ok, (0, 22)), INVALID), ((view, p.desc(), ok, (9, 3)), INVALID),
              ((view, p.desc(), P(flags=2)), INVALID), ((view, p.desc(), P(flags=3)), INVALID),
              ((view, p.desc(), P(passes=4)), INVALID), ((view, p.desc(), P(normal_squarings=8)), INVALID),
              ((view, p.desc(), P(max_history=0.5)), INVALID), ((view, p.desc(), P(max_history=257.0)), INVALID), ((view, p.desc(), P(max_history=nan)), INVALID),
              ((view, p.desc(), P(min_history=0.5)), INVALID), ((view, p.desc(), P(min_history=257.0)), INVALID), ((view, p.desc(), P(min_history=nan)), INVALID),
              ((view, p.desc(), P(depth_tolerance=0.0)), INVALID), ((view, p.desc(), P(depth_tolerance=inf)), INVALID),
              ((view, p.desc(), P(depth_sharpness=-1.0)), INVALID), ((view, p.desc(), P(depth_sharpness=inf)), INVALID),
              ((view, p.desc(), P(luminance_sigma=-1.0)), INVALID), ((view, p.desc(), P(luminance_sigma=inf)), INVALID), ((view, p.desc(), P(luminance_sigma=nan)), INVALID),
              ((view, p.desc(), P(luminance_floor=0.0)), INVALID), ((view, p.desc(), P(luminance_floor=inf)), INVALID), ((view, p.desc(), P(luminance_floor=nan)), INVALID),
              ((view, p.desc(), P(jitter=(inf, 0.0))), INVALID), ((view, p.desc(), P(previous_jitter=(0.0, nan))), INVALID),
              ((bad_view, p.desc(), ok), INVALID), ((nan_view, p.desc(), ok), INVALID), ((zero_view, p.desc(), ok), INVALID),
              ((view, p.desc(denoised_irradiance=shaped("denoised_irradiance", width=68)), ok), INVALID), ((view, p.desc(depth=shaped("depth", height=20)), ok), INVALID),
              ((view, p.desc(ray_buffer=shaped("ray_buffer", width=0)), ok), INVALID),
              ((view, p.desc(moments_out=shaped("moments_out", row_pitch_bytes=554)), ok), INVALID),       # at least a row, but no multiple of 4
              ((view, p.desc(accum_out=shaped("accum_out", row_pitch_bytes=1100)), ok), INVALID),          # smaller than a row
              ((view, p.desc(normals=shaped("normals", ptr=pl["normals"].ptr + 2)), ok), INVALID),         # misaligned
              ((view, p.desc(accum_out=pl["history"]), ok), INVALID),        # in place: the taps read any row of the history
              ((view, p.desc(moments_out=pl["history_moments"]), ok), INVALID),
              ((view, p.desc(denoised_irradiance=pl["ray_irradiance"]), ok), INVALID), ((view, p.desc(denoised_ray_buffer=pl["ray_buffer"]), ok), INVALID),
              ((view, p.desc(denoised_irradiance=pl["denoised_ray_buffer"]), ok), INVALID), ((view, p.desc(denoised_ray_buffer=pl["normals"]), ok), INVALID)]
    for args, status in cases:
        with pytest.raises(lib.SahError) as e:
            hip_ctx.rtgi_denoise(*args)
        assert e.value.status == status, args
    torch.cuda.synchronize()
    assert all(im.unchanged() for im in p.images.values())


def test_history_invalid_flag_excuses_the_previous_planes(hip_ctx, fixture):
    inputs = gen.frame_of(fixture, 1)
    params = _params(**dict(gen.params(1, 3), flags=_abi.RTGI_DENOISE_HISTORY_INVALID))
    view = reprojection_view_data_of(gen.view(1))
    cut = dict(inputs, previous_depth=None, history=None, history_moments=None)
    without = Planes(cut)
    assert set(without.images) == set(NAMES) - set(PREVIOUS)
    got = without.run(hip_ctx, view, params)
    want = reference(cut, gen.view(1), dict(gen.params(1, 3), flags=ref.HISTORY_INVALID))
    assert_outputs(got, want)
    assert set(np.unique(got[0][..., 3])) == {0.0, 1.0}  # sample counts 0 (no surface) and 1
    bogus = _abi.Plane(4, 3, 3, 2, 0)  # neither read nor checked
    withp = Planes(inputs)
    hip_ctx.rtgi_denoise(view, withp.desc(previous_depth=bogus, history=bogus, history_moments=bogus), params)
    assert_outputs(withp.outputs(), want)


def test_side_stream_captured_graph_replayed_twice_and_no_side_effects(fixture):
    import torch
    with side_stream_context() as (ctx, s):
        view, params = reprojection_view_data_of(gen.view(1)), _params(**gen.params(1, 3))
        a = Planes(gen.frame_of(fixture, 1))
        desc = a.desc()
        state = context_state(ctx)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.rtgi_denoise(view, desc, params)
        s.synchronize()
        assert_outputs(a.outputs(), fixture_want(fixture, 1, 3))
        assert context_state(ctx) == state
        # one captured graph (temporal, then filter: a linear chain), replayed twice over other input contents
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.rtgi_denoise(view, desc, params)
        for seed in (77, 78):
            inputs = ref.random_inputs(gen.WIDTH, gen.HEIGHT, seed)
            b = Planes(inputs)
            for n, _ in INPUTS:
                a.images[n].t.copy_(b.images[n].t)
            for n, _ in OUTPUTS:
                a.images[n].t.fill_(SENTINEL)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            want = ref.denoise_ex(*[inputs[k] for k in ORDER], gen.view(1), gen.params(1, 3))
            assert_outputs(a.outputs(), want[:4], f"replay with seed {seed}")
            assert want[4]["history"].sum() > 200
        assert context_state(ctx) == state


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------------
def _frames(extents, seed):
    """per frame (w, h, jitter, ray_buffer, ray_irradiance, depth, normals, motion_vectors): a static camera under a moving jitter, each
    frame other rays over the surfaces of random_inputs"""
    jitters = [(0.25 * i - 0.375, 0.125 * i + 0.125) for i in range(len(extents))]
    out = []
    for i, (w, h) in enumerate(extents):
        new = i == 0 or extents[i - 1] != (w, h)
        base = ref.random_inputs(w, h, seed + 7 * w)
        rays = ref.random_inputs(w, h, seed + 100 + i)
        mv = np.zeros((h, w, 2), np.float16)
        mv[...] = np.array(jitters[i]) - np.array(jitters[i] if new else jitters[i - 1])
        out.append((w, h, jitters[i], rays["ray_buffer"], rays["ray_irradiance"], base["depth"], base["normals"], mv.view(np.uint16)))
    return out


def test_four_frames_through_the_python_wrapper(hip_ctx):
    """frame.RtgiDenoiser: the first frame without a history, then three that accumulate (a static camera under a moving jitter, odd
    width); reset() starts over"""
    import torch
    W, H = 75, 40
    dn = frame.RtgiDenoiser(hip_ctx, W, H, max_history=8.0, min_history=3.0)
    assert dn.params.passes == 3 and dn.params.luminance_sigma == 4.0 and dn.params.max_history == 8.0 and dn.params.min_history == 3.0
    frames = _frames([(W, H)] * 5, 900)
    accum = moments = previous_depth = None
    for i, (w, h, jitter, rays, irr, depth, normals, mv) in enumerate(frames):
        if i == 4:
            dn.reset()
        first = i in (0, 4)
        if first:
            mv = np.zeros_like(mv)
        view = moved_view(W, H, dolly=0.0, jitter=jitter)
        depth = depth * f32(1.0 + 0.001 * i)  # each frame another depth plane: the wrapper must keep the one before
        out = dn.denoise(view, util.to_torch(rays), util.to_torch(irr), torch.from_numpy(depth).cuda(), util.to_torch(normals), util.to_torch(mv), jitter)
        torch.cuda.synchronize()
        assert out[0] is dn.denoised_ray_buffer and out[1] is dn.denoised_irradiance
        settings = dict(max_history=8.0, min_history=3.0, jitter=jitter, previous_jitter=jitter if first else frames[i - 1][2],
                        flags=ref.HISTORY_INVALID if first else 0)
        accum, moments, drb, dirr, info = ref.denoise_ex(rays, irr, depth, normals, mv, previous_depth, accum, moments, ref.View(view), settings)
        got = [t.cpu().numpy().view(np.uint16) for t in out]
        assert same(got[0], drb), f"frame {i} ray buffer: " + differs(got[0], drb)
        assert same(got[1], dirr), f"frame {i} irradiance: " + differs(got[1], dirr)
        assert same(dn.accum[dn.current].cpu().numpy(), accum) and same(dn.moments[dn.current].cpu().numpy(), moments)
        assert info["history"].sum() == (0 if first else info["ok"].sum())
        assert float(accum[..., 3].max()) == (1 if first else i + 1)
        assert info["filter"][0]["luminance_active"].any() == (i in (2, 3))  # min_history = 3
        previous_depth = depth


@pytest.mark.parametrize("passes", [3, 0])
def test_four_frames_through_the_cpp_facade(tmp_path, passes):
    """sah::RtgiDenoiser: the façade's own SceneView forms the view block (jitter, previous jitter, last_frame_view), which comes back with
    each frame's two denoised planes; the fourth frame has another extent, so the denoiser re-creates its textures and starts without a
    history.  The program also checks that the RTGI's denoise is off by default and refused without the motion vectors."""
    import subprocess
    frames = _frames([(80, 36)] * 3 + [(45, 50)], 950)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(frames), passes], np.uint32).tobytes())
        for w, h, jitter, rays, irr, depth, normals, mv in frames:
            f.write(np.array([w, h], np.uint32).tobytes() + np.array(jitter, f32).tobytes() + rays.tobytes() + irr.tobytes() + depth.tobytes() + normals.tobytes() + mv.tobytes())
    subprocess.check_call([host_program("host_rtgi_denoise", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    at = 0
    accum = moments = previous_depth = None
    for i, (w, h, jitter, rays, irr, depth, normals, mv) in enumerate(frames):
        view = _abi.ViewData.from_buffer_copy(blob[at:at + 432])
        got_rb = np.frombuffer(blob[at + 432:at + 432 + w * h * 8], np.uint16).reshape(h, w, 4)
        got_ir = np.frombuffer(blob[at + 432 + w * h * 8:at + 432 + w * h * 16], np.uint16).reshape(h, w, 4)
        at += 432 + w * h * 16
        first = i in (0, 3)
        assert tuple(view.render_resolution) == (w, h) and tuple(view.jitter) == tuple(f32(j) for j in jitter)
        assert first or tuple(view.previous_jitter) == tuple(f32(j) for j in frames[i - 1][2])
        settings = dict(passes=passes, jitter=tuple(view.jitter), previous_jitter=tuple(view.jitter) if first else tuple(view.previous_jitter),
                        flags=ref.HISTORY_INVALID if first else 0)
        accum, moments, drb, dirr, info = ref.denoise_ex(rays, irr, depth, normals, mv, previous_depth, accum, moments, ref.View(view), settings)
        assert same(got_rb, drb), f"frame {i} ray buffer: " + differs(got_rb, drb)
        assert same(got_ir, dirr), f"frame {i} irradiance: " + differs(got_ir, dirr)
        assert info["history"].sum() == (0 if first else info["ok"].sum()) and info["ok"].mean() > 0.5
        previous_depth = depth
    assert at == len(blob)


# ---- the frame the pass exists for -------------------------------------------------------------------------------------------------------------
def test_atrium_rtgi_denoised_over_sixteen_frames_then_rtgi_lighting(hip_ctx):
    """sah_gbuffer_render and sah_motion_vectors_render of the atrium at 128 x 72, sah_rt_build, then 16 frames of sah_rtgi_trace, each with
    another noise plane, each followed by sah_rtgi_denoise (every frame equal to the restatement on the device's planes); sah_lighting in
    RTGI mode with num_extra_rays = 0 on the denoised pair equals the oracle lighting on the same planes, and differs from the frame lit from
    the raw pair; and against the mean of E over 256 further traces — the estimate of the converged cosine-weighted irradiance — the RMS
    error falls from the raw frame to accum_out to the denoised irradiance (orderings, not thresholds; the figures are printed and recorded
    in DESIGN.md section 5t: 4.684, 1.193, 0.482 on an MI355X)."""
    import torch
    from androidrenderer_amd import mesh
    from tests.test_rt import RtCase
    W, H = 128, 72
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    view = scene.SceneView.default(W, H)
    view.update_transforms()  # a static camera: the last frame's matrices are this frame's
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    gb = {k: torch.zeros((H, W) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
    mv_t = torch.zeros((H, W, 2), dtype=torch.int16, device="cuda")
    frame.rasterised_frame(hip_ctx, geo, view.gpu_data, gb, motion_vectors=mv_t)
    torch.cuda.synchronize()
    depth, normals, mv = gb["depth"].cpu().numpy(), gb["normals"].cpu().numpy().view(np.uint16), mv_t.cpu().numpy().view(np.uint16)
    case = RtCase(mesh.atrium(2), W, H, view=view, gbuffer={"depth": depth, "normals": normals})
    case.hip_build(hip_ctx)

    def trace(seed):
        case.device()["noise"] = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (128, 128, 4), dtype=np.uint8)).cuda()
        rb, ri = case.hip_rtgi(hip_ctx)
        return rb.view(np.uint16), ri.view(np.uint16)
    dn = frame.RtgiDenoiser(hip_ctx, W, H)
    accum = moments = None
    rview = ref.View(view.gpu_data)
    for i in range(16):
        rb, ri = trace(1000 + i)
        out = dn.denoise(view.gpu_data, util.to_torch(rb), util.to_torch(ri), gb["depth"], gb["normals"], mv_t, (0.0, 0.0))
        torch.cuda.synchronize()
        accum, moments, drb, dirr, info = ref.denoise_ex(rb, ri, depth, normals, mv, depth, accum, moments, rview, dict(flags=0 if i else ref.HISTORY_INVALID))
        got = [t.cpu().numpy().view(np.uint16) for t in out]
        assert same(got[0], drb), f"frame {i} ray buffer: " + differs(got[0], drb)
        assert same(got[1], dirr), f"frame {i} irradiance: " + differs(got[1], dirr)
        assert same(dn.accum[dn.current].cpu().numpy(), accum) and same(dn.moments[dn.current].cpu().numpy(), moments)
        n = accum[..., 3][info["ok"]]
        # (the rasteriser's motion vectors are its rounding, not 0: up to four taps, whose weighted mean of equal counts rounds; a tap across an
        # edge may be rejected)
        assert (n <= i + 1 + 1e-3).all() and (np.abs(n - (i + 1)) < 1e-3).mean() > 0.99
    covered = info["ok"]
    assert info["filter"][0]["luminance_active"][covered].mean() > 0.99
    N = ref.surfaces(depth, normals, rview)[3]
    converged = np.zeros((H, W, 3), np.float64)
    for k in range(256):
        converged += ref.sample(*trace(5000 + k), N)
    converged /= 256
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - converged)[covered] ** 2)))  # noqa: E731
    value = lambda bits: bits.view(np.float16)[..., :3].astype(f32)  # noqa: E731
    rms_raw, rms_accum, rms_denoised = rms(ref.sample(rb, ri, N)), rms(accum[..., :3]), rms(value(dirr))
    print(f"atrium {W} x {H}, RTGI at one ray a pixel, frame 16: {float(covered.mean()):.2f} covered, converged E mean {float(converged[covered].mean()):.5f}; "
          f"RMS error raw {rms_raw:.5f}, accum_out {rms_accum:.5f}, denoised {rms_denoised:.5f}")
    assert covered.mean() > 0.5 and rms_denoised < rms_accum < rms_raw
    f = util.LightingFrame(W, H, gbuffer={k: (v.cpu().numpy().view(np.uint16) if k == "normals" else v.cpu().numpy()) for k, v in gb.items()}, seed=3,
                           sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_RTGI, num_extra_rays=0)
    f.arrays["ray_buffer"], f.arrays["ray_irr"] = rb, ri
    from_raw = f.run_hip(hip_ctx)
    f.arrays["ray_buffer"], f.arrays["ray_irr"] = got[0], got[1]
    lit, oracle = f.run_hip(hip_ctx), f.run_oracle()
    d = util.f16_ulp_diff(lit, oracle)
    print(util.report_ulp("atrium, RTGI lighting on the denoised pair", d))
    assert d.max() == 0 and (lit != from_raw).any()
