"""GPU: sah_rt_denoise (include/sah_rt_denoise.h) against the numpy restatement (tests/rt_denoise_ref.py) run on the device's own planes,
and its committed fixture, bit for bit in all three outputs; the call's contract (row bands, refusals, NULL previous planes, a captured
graph); frame.RayTracedDenoiser and the C++ façade over successive frames; and the frame the pass exists for.  The temporal kernel's tile is
64 x 16 pixels, the filter kernel's 32 x 16."""
import faulthandler
import os
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, frame, lib, scene
from tests import rt_denoise_ref as ref
from tests import util
from tests.host_programs import host_program
from tests.support import context_state, differs, Image, reprojection_view_data_of, retyped, same, SENTINEL, side_stream_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_rt_denoise as gen  # noqa: E402

f32 = np.float32
D32, RGBA16F, RG16F, R32F, R16F = (_abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R16G16_SFLOAT, _abi.FORMAT_R32_SFLOAT,
                                   _abi.FORMAT_R16_SFLOAT)
INPUTS = (("noisy", R32F), ("depth", D32), ("normals", RGBA16F), ("motion_vectors", RG16F), ("previous_depth", D32), ("history", R32F),
          ("history_length", R16F))
OUTPUTS = (("accum_out", R32F), ("length_out", R16F), ("denoised", R32F))
NAMES = [n for n, _ in INPUTS + OUTPUTS]
ORDER = ("noisy", "depth", "normals", "motion_vectors", "previous_depth", "history", "history_length")


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
    return _abi.RtDenoiseParams.default(**changes)


def pitch_of(fmt, w):
    return (w * _abi.FORMAT_BPP[fmt] + 3) // 4 * 4  # the smallest pitch the argument check admits (R16F rows of odd width are padded)


class Planes:
    """the ten device planes of one call; `layout`: {name: (pitch, offset)} in bytes; `inputs`: the seven input planes by name (None: the
    plane is not created and NULL is passed)"""

    def __init__(self, inputs, layout=None):
        h, w = inputs["noisy"].shape
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
        return _abi.RtDenoiseDesc.of(**planes)

    def run(self, ctx, view_data, params, rows=(0, 0)):
        import torch
        ctx.rt_denoise(view_data, self.desc(), params, rows)
        torch.cuda.synchronize()
        assert all(self.images[n].unchanged() for n, _ in INPUTS if n in self.images)
        return self.outputs()

    def outputs(self):
        im = self.images
        return (im["accum_out"].texels(f32).reshape(self.h, self.w), im["length_out"].texels(np.uint16).reshape(self.h, self.w),
                im["denoised"].texels(f32).reshape(self.h, self.w))


def assert_outputs(got, want, what=""):
    for name, g, w in zip(("accum_out", "length_out", "denoised"), got, want):
        w = w.view(np.uint16) if w.dtype == np.float16 else w
        assert same(g, w), f"{what} {name}: " + differs(g, w)


def reference(inputs, view, settings):
    return ref.denoise(*[inputs.get(k) for k in ORDER], view, settings)


def fixture_want(fx, i, passes):
    return fx[f"accum{i}"], fx[f"length{i}"], fx[f"denoised{i}_passes{passes}"]


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 2, 3])
def test_fixture_bit_for_bit_and_repeatable(hip_ctx, fixture, passes):
    for i in range(gen.FRAMES):
        inputs, view, params = gen.frame_of(fixture, i), reprojection_view_data_of(gen.view(i)), _params(**gen.params(i, passes))
        got = Planes(inputs).run(hip_ctx, view, params)
        assert_outputs(got, fixture_want(fixture, i, passes), f"frame {i}")
        assert_outputs(Planes(inputs).run(hip_ctx, view, params), got, f"frame {i} again")


# ---- extents --------------------------------------------------------------------------------------------------------------------------------
# temporal tile 64 x 16, filter tile 32 x 16: one below, at and one above each in each axis; an odd extent of three temporal tiles by three
@pytest.mark.parametrize("extent", [(1, 1), (3, 2), (63, 15), (64, 16), (65, 17), (31, 16), (32, 17), (33, 15), (131, 37)])
@pytest.mark.parametrize("passes", [0, 1, 2, 3])
def test_extents(hip_ctx, extent, passes):
    w, h = extent
    inputs = ref.random_inputs(w, h, 7 * w + h)
    view = moved_view(w, h)
    settings = dict(passes=passes, jitter=(0.25, -0.125), previous_jitter=(-0.25, 0.375), max_history=24.0)
    got = Planes(inputs).run(hip_ctx, view, _params(**settings))
    accum, length, denoised, info = ref.denoise_ex(*[inputs[k] for k in ORDER], ref.View(view), settings)
    assert_outputs(got, (accum, length, denoised), f"{w} x {h}")
    if w * h >= 64:  # (not because nothing happens)
        assert info["history"].sum() > w * h // 8 and info["depth_rejected"].any() and (info["taps_valid"] > 1).any() and (~info["ok"]).any()
        assert passes == 0 or (denoised != accum).sum() > w * h // 4


# ---- pitches and alignment ----------------------------------------------------------------------------------------------------------------
def _layout(pad, offset):
    """every plane with `pad` bytes more than a row (rounded to the check's multiple of 4) and a base shifted by `offset`"""
    return {n: (pitch_of(f, gen.WIDTH) + pad, offset) for n, f in INPUTS + OUTPUTS}


LAYOUTS = {"dwords: nothing 16-byte aligned": _layout(4, 4),
           "16-byte path: padded, shifted by 32": {n: ((pitch_of(f, gen.WIDTH) + 31) // 16 * 16, 32) for n, f in INPUTS + OUTPUTS},
           "one input 8-byte aligned only": dict({n: ((pitch_of(f, gen.WIDTH) + 31) // 16 * 16, 0) for n, f in INPUTS + OUTPUTS},
                                                 motion_vectors=(288, 8)),
           "length_out off the 16-byte pitch": dict({n: ((pitch_of(f, gen.WIDTH) + 31) // 16 * 16, 0) for n, f in INPUTS + OUTPUTS},
                                                    length_out=(140, 0))}


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
    assembled = [np.full((H, W), SENTINEL, np.uint8).repeat(4, 1).view(f32), np.full((H, W), SENTINEL, np.uint8).repeat(2, 1).view(np.uint16),
                 np.full((H, W), SENTINEL, np.uint8).repeat(4, 1).view(f32)]
    for rows in ((9, 10), (0, 9), (10, H), (17, 19), (5, 5), (0, 1), (H - 1, H)):
        p = Planes(gen.frame_of(fixture, 1), _layout(12, 0))
        got = p.run(hip_ctx, view, params, rows)
        wide = ref.band_rows(rows, H, passes)
        for k, (name, _) in enumerate(OUTPUTS):
            r = rows if name == "denoised" else wide
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
    INVALID, FORMAT = _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
    P = lambda **kw: _params(**dict(gen.params(1, 3), **kw))  # noqa: E731
    inf = float("inf")
    cases = [((view, p.desc(**{n: retyped(pl[n], D32 if f != D32 else R32F)}), ok), FORMAT) for n, f in INPUTS + OUTPUTS]
    cases += [((view, p.desc(**{n: None}), ok), INVALID) for n in NAMES]  # a previous-frame plane may be NULL only with the flag
    cases += [((view, p.desc(), ok, (0, 22)), INVALID), ((view, p.desc(), ok, (9, 3)), INVALID),
              ((view, p.desc(), P(flags=2)), INVALID), ((view, p.desc(), P(flags=3)), INVALID),
              ((view, p.desc(), P(passes=4)), INVALID), ((view, p.desc(), P(normal_squarings=8)), INVALID),
              ((view, p.desc(), P(max_history=0.5)), INVALID), ((view, p.desc(), P(max_history=257.0)), INVALID), ((view, p.desc(), P(max_history=float("nan"))), INVALID),
              ((view, p.desc(), P(depth_tolerance=0.0)), INVALID), ((view, p.desc(), P(depth_tolerance=inf)), INVALID),
              ((view, p.desc(), P(depth_sharpness=-1.0)), INVALID), ((view, p.desc(), P(depth_sharpness=inf)), INVALID),
              ((view, p.desc(), P(jitter=(inf, 0.0))), INVALID), ((view, p.desc(), P(previous_jitter=(0.0, float("nan")))), INVALID),
              ((bad_view, p.desc(), ok), INVALID), ((nan_view, p.desc(), ok), INVALID),
              ((view, p.desc(denoised=shaped("denoised", width=68)), ok), INVALID), ((view, p.desc(depth=shaped("depth", height=20)), ok), INVALID),
              ((view, p.desc(noisy=shaped("noisy", width=0)), ok), INVALID),
              ((view, p.desc(history_length=shaped("history_length", row_pitch_bytes=138)), ok), INVALID),   # a row of 69 halfs, but no multiple of 4
              ((view, p.desc(accum_out=shaped("accum_out", row_pitch_bytes=272)), ok), INVALID),             # smaller than a row
              ((view, p.desc(normals=shaped("normals", ptr=pl["normals"].ptr + 2)), ok), INVALID),           # misaligned
              ((view, p.desc(accum_out=pl["history"]), ok), INVALID),        # in place: the taps read any row of the history
              ((view, p.desc(denoised=pl["noisy"]), ok), INVALID), ((view, p.desc(denoised=pl["accum_out"]), ok), INVALID),
              ((view, p.desc(length_out=pl["history_length"]), ok), INVALID)]
    for args, status in cases:
        with pytest.raises(lib.SahError) as e:
            hip_ctx.rt_denoise(*args)
        assert e.value.status == status, args
    torch.cuda.synchronize()
    assert all(im.unchanged() for im in p.images.values())


def test_history_invalid_flag_excuses_the_previous_planes(hip_ctx, fixture):
    inputs = gen.frame_of(fixture, 1)
    params = _params(**dict(gen.params(1, 3), flags=_abi.RT_DENOISE_HISTORY_INVALID))
    view = reprojection_view_data_of(gen.view(1))
    without = Planes(dict(inputs, previous_depth=None, history=None, history_length=None))
    assert set(without.images) == set(NAMES) - {"previous_depth", "history", "history_length"}
    got = without.run(hip_ctx, view, params)
    want = reference(dict(inputs, previous_depth=None, history=None, history_length=None), gen.view(1), dict(gen.params(1, 3), flags=ref.HISTORY_INVALID))
    assert_outputs(got, want)
    assert set(np.unique(got[1])) == {0, 0x3c00}  # lengths 0 and 1
    bogus = _abi.Plane(4, 3, 3, 2, 0)  # neither read nor checked
    withp = Planes(inputs)
    hip_ctx.rt_denoise(view, withp.desc(previous_depth=bogus, history=bogus, history_length=bogus), params)
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
            ctx.rt_denoise(view, desc, params)
        s.synchronize()
        assert_outputs(a.outputs(), fixture_want(fixture, 1, 3))
        assert context_state(ctx) == state
        # one captured graph (temporal, then filter: a linear chain), replayed twice over other input contents
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.rt_denoise(view, desc, params)
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
            assert_outputs(a.outputs(), want[:3], f"replay with seed {seed}")
            assert want[3]["history"].sum() > 200


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------------------
def test_four_frames_through_the_python_wrapper(hip_ctx):
    """frame.RayTracedDenoiser: the first frame without a history, then three that accumulate (a static camera under a moving jitter, odd
    width: the wrapper pads the rows of its length planes); reset() starts over"""
    import torch
    W, H = 75, 40
    dn = frame.RayTracedDenoiser(hip_ctx, W, H, max_history=8.0)
    assert dn.params.passes == 3 and dn.params.normal_squarings == 5 and dn.params.max_history == 8.0
    base = ref.random_inputs(W, H, 900)
    jitters = [(0.25 * i - 0.375, 0.125 * i + 0.125) for i in range(5)]
    accum = length = previous_depth = None
    for i, jitter in enumerate(jitters):
        if i == 4:
            dn.reset()
        first = i in (0, 4)
        view = moved_view(W, H, dolly=0.0, jitter=jitter)
        noisy = (np.random.default_rng(50 + i).random((H, W)) < 0.5).astype(f32)
        mv = np.zeros((H, W, 2), np.float16)
        mv[...] = np.array(jitter) - np.array(jitters[i - 1] if not first else jitter)
        depth = base["depth"] * f32(1.0 + 0.01 * i)  # each frame another depth plane: the wrapper must keep the one before
        out = dn.denoise(view, torch.from_numpy(noisy).cuda(), torch.from_numpy(depth).cuda(), util.to_torch(base["normals"]),
                         util.to_torch(mv.view(np.uint16)), jitter)
        torch.cuda.synchronize()
        assert out is dn.denoised
        settings = dict(max_history=8.0, jitter=jitter, previous_jitter=jitter if first else jitters[i - 1], flags=ref.HISTORY_INVALID if first else 0)
        accum, length, want, info = ref.denoise_ex(noisy, depth, base["normals"], mv, previous_depth, accum, length, ref.View(view), settings)
        assert same(out.cpu().numpy(), want), f"frame {i}: " + differs(out.cpu().numpy(), want)
        assert same(dn.accum[dn.current].cpu().numpy(), accum) and same(dn.length[dn.current].cpu().numpy()[:, :W], length)
        assert info["history"].sum() == (0 if first else info["ok"].sum())
        assert float(length.max()) == (1 if first else i + 1)
        previous_depth = depth


@pytest.mark.parametrize("passes", [3, 0])
def test_four_frames_through_the_cpp_facade(tmp_path, passes):
    """sah::RayTracedDenoiser: the façade's own SceneView forms the view block (jitter, previous jitter, last_frame_view), which comes back
    with each denoised plane; the fourth frame has another extent, so the denoiser re-creates its textures and starts without a history.
    The program also checks that the AO phase's denoise is off by default and refused without an allocator."""
    import subprocess
    extents = [(80, 36)] * 3 + [(45, 50)]
    jitters = [(0.25 * i - 0.375, 0.125 * i + 0.125) for i in range(len(extents))]
    frames = []
    for i, (w, h) in enumerate(extents):
        base = ref.random_inputs(w, h, 950 + (i == 3))
        noisy = (np.random.default_rng(60 + i).random((h, w)) < 0.5).astype(f32)
        mv = np.zeros((h, w, 2), np.float16)
        mv[...] = np.array(jitters[i]) - np.array(jitters[i - 1] if i else jitters[i])
        frames.append((w, h, jitters[i], noisy, base["depth"], base["normals"], mv.view(np.uint16)))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(frames), passes], np.uint32).tobytes())
        for w, h, jitter, noisy, depth, normals, mv in frames:
            f.write(np.array([w, h], np.uint32).tobytes() + np.array(jitter, f32).tobytes() + noisy.tobytes() + depth.tobytes() + normals.tobytes() + mv.tobytes())
    subprocess.check_call([host_program("host_rt_denoise", tmp_path), str(inp), str(outp)], timeout=120)
    blob = open(outp, "rb").read()
    at = 0
    accum = length = previous_depth = None
    for i, (w, h, jitter, noisy, depth, normals, mv) in enumerate(frames):
        view = _abi.ViewData.from_buffer_copy(blob[at:at + 432])
        facade = np.frombuffer(blob[at + 432:at + 432 + w * h * 4], f32).reshape(h, w)
        at += 432 + w * h * 4
        first = i in (0, 3)
        assert tuple(view.render_resolution) == (w, h) and tuple(view.jitter) == tuple(f32(j) for j in jitter)
        assert first or tuple(view.previous_jitter) == tuple(f32(j) for j in jitters[i - 1])
        settings = dict(passes=passes, jitter=tuple(view.jitter), previous_jitter=tuple(view.jitter) if first else tuple(view.previous_jitter),
                        flags=ref.HISTORY_INVALID if first else 0)
        accum, length, want, info = ref.denoise_ex(noisy, depth, normals, mv, previous_depth, accum, length, ref.View(view), settings)
        assert same(facade, want), f"frame {i}: " + differs(facade, want)
        assert info["history"].sum() == (0 if first else info["ok"].sum()) and info["ok"].mean() > 0.5
        previous_depth = depth
    assert at == len(blob)


# ---- the frame the pass exists for -------------------------------------------------------------------------------------------------------------
def test_atrium_rtao_denoised_over_sixteen_frames_then_lpv_lighting(hip_ctx):
    """sah_gbuffer_render and sah_motion_vectors_render of the atrium at 128 x 72, sah_rt_build, then 16 frames of sah_rtao at 1 spp, each
    with another noise plane, each followed by sah_rt_denoise (every frame equal to the restatement on the device's planes); sah_lighting in
    LPV mode on the denoised plane equals the oracle lighting on the same plane; and against the mean of sah_rtao over 256 further noise
    planes — the estimate of the converged AO — the RMS error falls from the raw frame to accum_out to `denoised` (orderings, not
    thresholds; the figures are printed and recorded in DESIGN.md section 5r: 0.4670, 0.1179, 0.0453 on an MI355X)."""
    import torch
    from androidrenderer_amd import images, mesh
    W, H = 128, 72
    keep = []
    geo = mesh.geometry(mesh.to_device(mesh.atrium(2).arrays()), keep)
    view = scene.SceneView.default(W, H)
    view.update_transforms()  # a static camera: the last frame's matrices are this frame's
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    gb = {k: torch.zeros((H, W) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
    mv_t = torch.zeros((H, W, 2), dtype=torch.int16, device="cuda")
    frame.rasterised_frame(hip_ctx, geo, view.gpu_data, gb, motion_vectors=mv_t)
    hip_ctx.rt_build(geo)
    torch.cuda.synchronize()
    depth, normals, mv = gb["depth"].cpu().numpy(), gb["normals"].cpu().numpy().view(np.uint16), mv_t.cpu().numpy().view(np.uint16)
    assert np.abs(mv.view(np.float16).astype(f32)).max() < 0.01  # a static camera: the vectors are the rasteriser's rounding, not 0
    raw_t = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    d_p, n_p, raw_p = images.plane(gb["depth"], D32), images.plane(gb["normals"], RGBA16F), images.plane(raw_t, R32F)

    def rtao(seed):
        noise = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (128, 128, 4), dtype=np.uint8)).cuda()
        hip_ctx.rtao(view.gpu_data, d_p, n_p, images.plane(noise, _abi.FORMAT_R8G8B8A8_UNORM), 1, 8.0, raw_p)
        torch.cuda.synchronize()
        return raw_t.cpu().numpy()
    dn = frame.RayTracedDenoiser(hip_ctx, W, H)
    accum = length = None
    rview = ref.View(view.gpu_data)
    for i in range(16):
        raw = rtao(1000 + i)
        assert set(np.unique(raw).tolist()) <= {0.0, 1.0}  # one noise texel for every ray of a pixel: binary
        out = dn.denoise(view.gpu_data, raw_t, gb["depth"], gb["normals"], mv_t, (0.0, 0.0))
        torch.cuda.synchronize()
        accum, length, want, info = ref.denoise_ex(raw, depth, normals, mv, depth, accum, length, rview, dict(flags=0 if i else ref.HISTORY_INVALID))
        got = out.cpu().numpy()
        assert same(got, want), f"frame {i}: " + differs(got, want)
        assert same(dn.accum[dn.current].cpu().numpy(), accum) and same(dn.length[dn.current].cpu().numpy()[:, :W], length)
        assert (length[info["ok"]] <= i + 1).all() and (length[info["ok"]] == i + 1).mean() > 0.99  # (a tap across an edge may be rejected)
    covered = info["ok"]
    converged = np.zeros((H, W), np.float64)
    for k in range(256):
        converged += rtao(5000 + k)
    converged /= 256
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - converged)[covered] ** 2)))  # noqa: E731
    rms_raw, rms_accum, rms_denoised = rms(raw), rms(accum), rms(got)
    print(f"atrium {W} x {H}, RTAO at 1 spp, frame 16: {float(covered.mean()):.2f} covered, converged AO mean {float(converged[covered].mean()):.3f}; "
          f"RMS error raw {rms_raw:.4f}, accum_out {rms_accum:.4f}, denoised {rms_denoised:.4f}")
    assert covered.mean() > 0.5 and rms_denoised < rms_accum < rms_raw
    f = util.LightingFrame(W, H, gbuffer={k: (v.cpu().numpy().view(np.uint16) if k == "normals" else v.cpu().numpy()) for k, v in gb.items()}, seed=3,
                           sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV)
    flat = f.run_hip(hip_ctx)  # the synthetic AO plane the frame had before: the AO plane matters to the result
    f.arrays["ao"] = got
    lit, oracle = f.run_hip(hip_ctx), f.run_oracle()
    d = util.f16_ulp_diff(lit, oracle)
    print(util.report_ulp("atrium, LPV lighting on the denoised RTAO plane", d))
    assert d.max() == 0 and (lit != flat).any()
