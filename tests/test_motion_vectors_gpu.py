"""The motion-vectors pass on the GPU (include/sah_motion_vectors.h): bit for bit against the numpy restatement on its fixture; exact zeros
where no SOLID fragment wins; padded pitches; no side effects on `depth`, the G-buffer, shadow and RSM passes; repeatability; and, for
clipped geometry and at full size, against the fp64 reprojection of every SOLID-won pixel (tests/mv_reproject.py).

Every GPU step runs under a watchdog of its own (`_limit`): a step that overruns ends the process, nothing is retried."""
import contextlib
import faulthandler
import math
import os
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, mesh, scene
from tests import mv_reproject, util
from tests.test_lpv_inject import _hip_rsm, _setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_motion_vectors as gmv  # noqa: E402

# The tolerance of the reprojection check is measured on the fixture (DESIGN.md §7 "Motion vectors"; tests/mv_reproject.py holds the
# figures and tests/test_motion_vectors_cpu.py recomputes them): a pixel is kept when its two components lie within
# DEVIATION_FACTOR x FIXTURE_EXCESS_PIXELS + half an fp16 spacing of the fp64 reprojection AND within DEVIATION_FACTOR x
# FIXTURE_DEVIATION_SPACINGS spacings of the fp16 grid at the stored value; at most MAX_LEFT_OUT of the SOLID-won pixels are not.
from tests.mv_reproject import DEVIATION_FACTOR, FIXTURE_DEVIATION_SPACINGS, FIXTURE_EXCESS_PIXELS, MAX_LEFT_OUT  # noqa: E402


@contextlib.contextmanager
def _limit(seconds):
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


FORMATS = {"color": _abi.FORMAT_R8G8B8A8_SRGB, "normals": _abi.FORMAT_R16G16B16A16_SFLOAT, "data": _abi.FORMAT_R8G8B8A8_UNORM,
           "emission": _abi.FORMAT_R8G8B8A8_SRGB, "depth": _abi.FORMAT_D32_SFLOAT}


def _plane(t, W, fmt):
    """the first W texels of every row of a (H, W + padding[, C]) device array"""
    return _abi.Plane(t.data_ptr(), W, t.shape[0], t.stride(0) * t.element_size(), fmt)


def _targets(W, H, pad=0):
    import torch
    shapes = {"color": (4, torch.uint8), "normals": (4, torch.int16), "data": (4, torch.uint8), "emission": (4, torch.uint8), "depth": (0, torch.float32)}
    full = {k: torch.zeros((H, W + pad) + ((c,) if c else ()), dtype=t, device="cuda") for k, (c, t) in shapes.items()}
    return full, {k: v[:, :W] for k, v in full.items()}


def _gbuffer(ctx, geo, view, W, H, pad=0, stats=None):
    import torch
    full, gb = _targets(W, H, pad)
    with _limit(120):
        ctx.gbuffer_render(geo, view.gpu_data, _abi.GBuffer(*[_plane(full[k], W, FORMATS[k]) for k in ("color", "normals", "data", "emission", "depth")]), stats)
        torch.cuda.synchronize()
    return full, gb


def _motion(ctx, geo, view, depth, W, H, pad=0, fill=0x5A5A):
    import torch
    full = torch.full((H, W + pad, 2), fill, dtype=torch.int16, device="cuda")
    with _limit(120):
        ctx.motion_vectors_render(geo, view.gpu_data, _plane(depth, W, _abi.FORMAT_D32_SFLOAT), _plane(full, W, _abi.FORMAT_R16G16_SFLOAT))
        torch.cuda.synchronize()
    return util.from_torch(full, np.uint16).reshape(H, W + pad, 2)


def _moved_view(W, H, position=(-7.0, 1.0, 0.0)):
    """a camera that moved, turned and changed its jitter between the last frame and this one"""
    v = scene.SceneView()
    v.set_render_resolution(W, H)
    v.set_perspective_projection(75.0, float(W) / float(H), 0.05)
    v.rotate(0.0, math.radians(90.0))
    v.set_position(position)
    v.jitter = np.array([0.3, -0.2], np.float32)
    v.update_transforms()
    v.rotate(0.02, 0.03)
    v.set_position([position[0] - 0.3, position[1] + 0.1, position[2] + 0.2])
    v.jitter = np.array([-0.25, 0.4], np.float32)
    v.update_transforms()
    return v


def _fixture_on_gpu(hip_ctx, pad=0):
    fx = np.load(gmv.FIXTURE)
    m, view = gmv.fixture_scene(int(fx["seed"]))
    keep = []
    geo = mesh.geometry(mesh.to_device(m.arrays()), keep)
    full, gb = _gbuffer(hip_ctx, geo, view, gmv.WIDTH, gmv.HEIGHT, pad)
    return fx, m, view, geo, keep, full, gb


def _same_bits(got, want):
    g16, w16 = got.view(np.float16), want.view(np.float16)
    nan = np.isnan(g16) | np.isnan(w16)
    return np.array_equal(np.isnan(g16), np.isnan(w16)) and np.array_equal(got[~nan], want[~nan])


def test_fixture_bit_for_bit(hip_ctx):
    fx, m, view, geo, keep, full, gb = _fixture_on_gpu(hip_ctx)
    depth = util.from_torch(gb["depth"], np.float32).reshape(gmv.HEIGHT, gmv.WIDTH)
    assert np.array_equal(depth.view(np.uint32), fx["depth"].view(np.uint32)), "the G-buffer depth differs from the fixture's"
    got = _motion(hip_ctx, geo, view, gb["depth"], gmv.WIDTH, gmv.HEIGHT)
    bad = (got != fx["motion_vectors"]).any(-1)
    assert _same_bits(got, fx["motion_vectors"]), f"{int(bad.sum())} texels differ, first at {np.argwhere(bad)[:4].tolist()}"
    assert (got[fx["solid_won"]] != 0).any()


def test_sky_and_cutout_won_pixels_are_exactly_zero(hip_ctx):
    fx, m, view, geo, keep, full, gb = _fixture_on_gpu(hip_ctx)
    got = _motion(hip_ctx, geo, view, gb["depth"], gmv.WIDTH, gmv.HEIGHT)
    # the G-buffer winner is CUTOUT where the depth differs from the depth of the SOLID primitives alone
    arrays = m.arrays()
    arrays["primitives"] = arrays["primitives"][arrays["primitives"]["type"] == _abi.PRIMITIVE_TYPE_SOLID]
    keep2 = []
    solid_geo = mesh.geometry(mesh.to_device(arrays), keep2)
    _, solid_gb = _gbuffer(hip_ctx, solid_geo, view, gmv.WIDTH, gmv.HEIGHT)
    depth = util.from_torch(gb["depth"], np.float32).reshape(gmv.HEIGHT, gmv.WIDTH)
    solid_depth = util.from_torch(solid_gb["depth"], np.float32).reshape(gmv.HEIGHT, gmv.WIDTH)
    sky, cutout = depth == 0, depth != solid_depth
    assert sky.sum() > 100 and cutout.sum() > 100 and not (sky & cutout).any()
    assert (got[sky] == 0).all() and (got[cutout] == 0).all()
    assert np.array_equal(~(sky | cutout), fx["solid_won"])


def test_padded_pitches_give_the_same_texels_and_leave_the_padding(hip_ctx):
    W, H = gmv.WIDTH, gmv.HEIGHT
    fx, m, view, geo, keep, full, gb = _fixture_on_gpu(hip_ctx, pad=24)
    import torch
    full["depth"][:, W:] = 0.625  # padding of the depth plane: never read as a texel
    torch.cuda.synchronize()
    got = _motion(hip_ctx, geo, view, gb["depth"], W, H, pad=40, fill=0x5A5A)
    assert _same_bits(np.ascontiguousarray(got[:, :W]), fx["motion_vectors"])
    assert (got[:, W:] == 0x5A5A).all()
    assert (util.from_torch(full["depth"], np.float32).reshape(H, W + 24)[:, W:] == 0.625).all()


def test_no_side_effects_on_depth_gbuffer_shadow_and_rsm(hip_ctx):
    import torch
    W, H = 640, 360
    view = _moved_view(W, H)
    arrays = mesh.random_soup(41, triangles=800, extent=8.0).arrays()
    keep = []
    geo = mesh.geometry(mesh.to_device(arrays), keep)
    _, gb = _gbuffer(hip_ctx, geo, view, W, H)
    before = {k: v.clone() for k, v in gb.items()}
    _, sun, lpv = _setup(W, H)
    sun.update_shadow_cascades(view, resolution=512)

    def shadow():
        sm = torch.full((4, 512, 512), 7, dtype=torch.int16, device="cuda")
        with _limit(120):
            hip_ctx.shadow_render(geo, sun.constants, 4, images.volume(sm, _abi.FORMAT_D16_UNORM))
            torch.cuda.synchronize()
        return sm
    def rsm():
        with _limit(120):
            out = _hip_rsm(hip_ctx, arrays, sun, lpv)
            torch.cuda.synchronize()
        return out
    sm0, rsm0 = shadow(), rsm()
    mv0 = _motion(hip_ctx, geo, view, gb["depth"], W, H)
    assert torch.equal(gb["depth"], before["depth"]), "the call wrote to its depth plane"
    sm1 = shadow()
    mv1 = _motion(hip_ctx, geo, view, gb["depth"], W, H)
    rsm1 = rsm()
    mv2 = _motion(hip_ctx, geo, view, gb["depth"], W, H)
    _, again = _gbuffer(hip_ctx, geo, view, W, H)
    assert torch.equal(sm0, sm1) and all(torch.equal(rsm0[k], rsm1[k]) for k in rsm0)
    assert all(torch.equal(before[k], again[k]) for k in before), "sah_gbuffer_render after the new call writes other planes"
    # two calls, and calls interleaved with the other rasteriser passes, give identical bytes.  (A captured-and-replayed call is not
    # compared: sah_gbuffer_render reads the rasteriser's counters back behind a stream synchronisation, which a capture forbids, and the
    # new call synchronises in the same place — neither is capturable on any scene.)
    assert np.array_equal(mv0, mv1) and np.array_equal(mv0, mv2)
    assert (mv0 != 0).any()


def _check_against_reprojection(hip_ctx, W, H, label):
    import torch
    m = mesh.atrium(8)
    view = _moved_view(W, H, position=(0.0, 1.0, 0.0))  # inside the atrium: its floor and walls cross the near plane
    keep = []
    geo = mesh.geometry(mesh.to_device(m.arrays()), keep)
    stats = torch.zeros(8, dtype=torch.int32, device="cuda")
    _, gb = _gbuffer(hip_ctx, geo, view, W, H, stats=stats.data_ptr())
    st = stats.cpu().numpy().astype(np.int64)
    assert st[0] == 23808
    assert st[3] > st[0] - st[1] - st[2], "no triangle of this frame was clipped into a fan"
    got = _motion(hip_ctx, geo, view, gb["depth"], W, H)
    depth = util.from_torch(gb["depth"], np.float32).reshape(H, W)
    solid = depth > 0  # every primitive of the atrium is SOLID
    assert solid.mean() > 0.5 and (got[~solid] == 0).all()
    want = mv_reproject.reproject(view.gpu_data, depth)
    spacings = mv_reproject.deviation_in_half_spacings(got, want, solid).max(-1)
    excess = mv_reproject.excess_over_store_rounding(got, want, solid).max(-1)
    allowed_spacings, allowed_excess = DEVIATION_FACTOR * FIXTURE_DEVIATION_SPACINGS, DEVIATION_FACTOR * FIXTURE_EXCESS_PIXELS
    with np.errstate(invalid="ignore"):
        kept = solid & (spacings <= allowed_spacings) & (excess <= allowed_excess)  # a NaN on either side is not kept
    left_out = int((solid & ~kept).sum())
    absdev = np.abs(got.view(np.float16).astype(np.float64) - want)[solid]
    print(f"{label}: {int(solid.sum())} SOLID-won pixels; kept: worst excess over the store's rounding {excess[kept].max():.5f} pixel (allowed "
          f"{allowed_excess:.5f}), worst {spacings[kept].max():.1f} spacings (allowed {allowed_spacings:.1f}); left out {left_out} "
          f"({100.0 * left_out / solid.sum():.4f} %: {int((solid & ~(excess <= allowed_excess)).sum())} by the excess, "
          f"{int((solid & ~(spacings <= allowed_spacings)).sum())} by the spacings); over all: excess 99th percentile {np.nanpercentile(excess[solid], 99):.5f}, "
          f"worst {np.nanmax(excess[solid]):.5f}, worst absolute {np.nanmax(absdev):.5f} pixel, median {np.nanmedian(absdev):.6f}, "
          f"largest |mv| {np.nanmax(np.abs(want[solid])):.2f}")
    assert left_out <= MAX_LEFT_OUT * solid.sum()


def test_clipped_geometry_against_fp64_reprojection(hip_ctx):
    _check_against_reprojection(hip_ctx, 1280, 720, "clipped 1280x720")


def test_4k_call_against_fp64_reprojection(hip_ctx):
    _check_against_reprojection(hip_ctx, 3840, 2160, "4K")


def _dense_soup_motion(ctx):
    """1500 large triangles piled on a 128 x 128 view (tests/test_raster.py: every tile's bin list has > 256 entries): G-buffer, then the
    motion vectors with their rasteriser counters"""
    import torch
    W = H = 128
    arrays = mesh.random_soup(31, triangles=1500, extent=1.5, size=(1.5, 4.0)).arrays()
    view = _moved_view(W, H, position=(0.0, 0.0, 0.0))
    keep = []
    geo = mesh.geometry(mesh.to_device(arrays), keep)
    _, gb = _gbuffer(ctx, geo, view, W, H)
    stats = torch.zeros(8, dtype=torch.int32, device="cuda")
    full = torch.full((H, W, 2), 0x5A5A, dtype=torch.int16, device="cuda")
    with _limit(120):
        ctx.motion_vectors_render(geo, view.gpu_data, _plane(gb["depth"], W, _abi.FORMAT_D32_SFLOAT), _plane(full, W, _abi.FORMAT_R16G16_SFLOAT), stats.data_ptr())
        torch.cuda.synchronize()
    covered = util.from_torch(gb["depth"], np.float32).reshape(H, W) > 0  # by a SOLID or a CUTOUT fragment
    return util.from_torch(full, np.uint16).reshape(H, W, 2), stats.cpu().numpy().astype(np.int64), covered


def test_split_bin_lists_merge_to_what_whole_lists_give(hip_ctx, monkeypatch):
    """Long bin lists are split into parts (k_split) whose "latest sequence number that matched" is merged by the last part to finish;
    SAH_RASTER_MERGE_CAPACITY=0 (testing hook, read at context creation) leaves every list whole, walked by one workgroup in rounds of 256
    entries.  Both paths run — [5] counts the extra parts handed out, [6] the tiles whose list is longer than one part — and give the
    same bytes."""
    import torch
    from androidrenderer_amd import lib
    split, split_stats, covered = _dense_soup_motion(hip_ctx)
    assert split_stats[5] > 0 and split_stats[6] >= 1 and split_stats[4] > 4 * 256
    monkeypatch.setenv("SAH_RASTER_MERGE_CAPACITY", "0")
    ctx = lib.Context(device=0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        whole, whole_stats, _ = _dense_soup_motion(ctx)
    finally:
        torch.cuda.synchronize()
        ctx.close()
    assert whole_stats[5] == 0 and whole_stats[6] >= 1 and list(whole_stats[:5]) == list(split_stats[:5])
    assert (split != 0).any(-1).mean() > 0.25 and (split[~covered] == 0).all()
    assert np.array_equal(split, whole)
