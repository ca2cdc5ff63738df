"""sah_gbuffer_motion_render on the GPU (include/sah_gbuffer_motion.h): the call IS sah_gbuffer_render followed by
sah_motion_vectors_render against the depth it wrote, so every test renders three ways on one context and compares BYTES over the whole
allocations, padding included: the fused call, the two calls, and for the G-buffer planes sah_gbuffer_render alone.  Both stand-alone
entries are held to the oracle, the golden fixture and the exact integer reference elsewhere; no further reference is needed here.

Every target is filled with a pattern first (0x5A5A for the motion plane, the byte 0xA7 for the G-buffer planes).  Every GPU step runs
under a watchdog of its own (`_limit`): a step that overruns ends the process, nothing is retried."""
import contextlib
import faulthandler
import os
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, lib, mesh
from tests import raster_exact_ref as ex
from tests import raster_ties_util as rt
from tests.test_lpv_inject import _hip_rsm, _setup
from tests.test_motion_vectors_gpu import _moved_view, _same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_motion_vectors as gmv  # noqa: E402

GB_BYTE, MV_BYTE = 0xA7, 0x5A  # (the motion plane reads 0x5A5A)
# plane, channels, torch dtype name, bytes per texel, format
PLANES = (("color", 4, "uint8", 4, _abi.FORMAT_R8G8B8A8_SRGB), ("normals", 4, "int16", 8, _abi.FORMAT_R16G16B16A16_SFLOAT),
          ("data", 4, "uint8", 4, _abi.FORMAT_R8G8B8A8_UNORM), ("emission", 4, "uint8", 4, _abi.FORMAT_R8G8B8A8_SRGB),
          ("depth", 0, "float32", 4, _abi.FORMAT_D32_SFLOAT), ("motion_vectors", 2, "int16", 4, _abi.FORMAT_R16G16_SFLOAT))
BPP = {name: bpp for name, _, _, bpp, _ in PLANES}
GBUFFER = tuple(name for name, *_ in PLANES[:5])
OFFSET = (1, 2)  # of a pitched plane in its allocation: rows, texels


@contextlib.contextmanager
def _limit(seconds=120):
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _origin(pad):
    return OFFSET if pad else (0, 0)


def _allocate(W, H, pad):
    """the six targets, pattern-filled: {name: device tensor (H [+ 2], W + pad [, channels])} and their planes of W x H texels, which start
    OFFSET into a padded allocation"""
    import torch
    row0, col0 = _origin(pad)
    full, planes = {}, {}
    for name, channels, dtype, bpp, fmt in PLANES:
        t = torch.zeros((H + 2 * row0, W + pad) + ((channels,) if channels else ()), dtype=getattr(torch, dtype), device="cuda")
        t.view(torch.uint8).fill_(GB_BYTE if name != "motion_vectors" else MV_BYTE)
        pitch = t.stride(0) * t.element_size()
        full[name], planes[name] = t, _abi.Plane(t.data_ptr() + row0 * pitch + col0 * bpp, W, H, pitch, fmt)
    return full, planes


def _render(ctx, geo, vd, W, H, how, pad=0):
    """how: 'fused' (the new call), 'two' (sah_gbuffer_render, sah_motion_vectors_render) or 'gbuffer' (the first alone).  Returns the
    whole allocations as bytes {name: (rows, pitch) uint8} and the eight statistics words."""
    import torch
    full, p = _allocate(W, H, pad)
    gb = _abi.GBuffer(*[p[k] for k in GBUFFER])
    stats = torch.full((_abi.RASTER_STATS_WORDS,), -1, dtype=torch.int32, device="cuda")
    with _limit():
        if how == "fused":
            ctx.gbuffer_motion_render(geo, vd, gb, p["motion_vectors"], stats.data_ptr())
        else:
            ctx.gbuffer_render(geo, vd, gb, stats.data_ptr())
            if how == "two":
                ctx.motion_vectors_render(geo, vd, p["depth"], p["motion_vectors"])
        torch.cuda.synchronize()
    out = {k: v.view(torch.uint8).reshape(v.shape[0], -1).cpu().numpy() for k, v in full.items()}
    return out, stats.cpu().numpy().astype(np.int64)


def _texels(out, name, W, H, pad=0):
    """the W x H texels of a plane as (H, W, bytes per texel) uint8, and whether every byte around them still holds its pattern"""
    row0, col0 = _origin(pad)
    a, bpp = out[name], BPP[name]
    inside = np.zeros(a.shape, bool)
    inside[row0:row0 + H, col0 * bpp:(col0 + W) * bpp] = True
    pattern = MV_BYTE if name == "motion_vectors" else GB_BYTE
    return a[inside].reshape(H, W, bpp), bool((a[~inside] == pattern).all())


def _motion(out, W, H, pad=0):
    return np.ascontiguousarray(_texels(out, "motion_vectors", W, H, pad)[0]).view(np.uint16).reshape(H, W, 2)


def _depth(out, W, H, pad=0):
    return np.ascontiguousarray(_texels(out, "depth", W, H, pad)[0]).view(np.float32).reshape(H, W)


def _assert_same(a, b, what, names=tuple(n for n, *_ in PLANES)):
    for k in names:
        bad = np.argwhere(a[k] != b[k])
        assert bad.size == 0, f"{what}: plane '{k}': {len(bad)} bytes differ, first at (row, byte) {bad[0].tolist()}: {a[k][tuple(bad[0])]} against {b[k][tuple(bad[0])]}"


def _three_ways(ctx, geo, vd, W, H, what, pad=0):
    """fused, two calls, G-buffer alone on `ctx`: asserts the composition contract and returns (fused, statistics)"""
    fused, st_f = _render(ctx, geo, vd, W, H, "fused", pad)
    two, st_t = _render(ctx, geo, vd, W, H, "two", pad)
    alone, st_a = _render(ctx, geo, vd, W, H, "gbuffer", pad)
    _assert_same(fused, two, f"{what}: the fused call against the two calls")
    _assert_same(fused, alone, f"{what}: the fused call against sah_gbuffer_render alone", GBUFFER)
    assert (alone["motion_vectors"] == MV_BYTE).all()
    assert list(st_f) == list(st_t) == list(st_a), f"{what}: statistics {list(st_f)} against sah_gbuffer_render's {list(st_a)}"
    for name, *_ in PLANES:
        assert _texels(fused, name, W, H, pad)[1], f"{what}: plane '{name}': bytes outside the texels were written"
    return fused, st_f


def _device(arrays):
    return mesh.geometry(mesh.to_device(arrays), [])


def _new_ctx():
    import torch
    ctx = lib.Context(device=0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return ctx


@pytest.fixture
def fresh_ctx():
    import torch
    ctx = _new_ctx()
    yield ctx
    torch.cuda.synchronize()
    ctx.close()


_fixture_cache = {}


def _fixture(hip_ctx):
    """the 96 x 54 motion fixture, rendered the three ways once per session: (fixture arrays, geometry, view data, fused planes, statistics)"""
    if not _fixture_cache:
        fx = np.load(gmv.FIXTURE)
        m, view = gmv.fixture_scene(int(fx["seed"]))
        geo = _device(m.arrays())
        fused, stats = _three_ways(hip_ctx, geo, view.gpu_data, gmv.WIDTH, gmv.HEIGHT, "fixture")
        _fixture_cache["v"] = (fx, geo, view.gpu_data, fused, stats)
    return _fixture_cache["v"]


# ---- 1, 2: the fixture, tight and pitched -------------------------------------------------------------------------------------------------
def test_fixture_equals_the_two_calls_and_the_golden_motion_vectors(hip_ctx):
    fx, geo, vd, fused, stats = _fixture(hip_ctx)
    W, H = gmv.WIDTH, gmv.HEIGHT
    got = _motion(fused, W, H)
    bad = (got != fx["motion_vectors"]).any(-1)
    assert _same_bits(got, fx["motion_vectors"]), f"{int(bad.sum())} texels differ from the fixture, first at {np.argwhere(bad)[:4].tolist()}"
    assert np.array_equal(_depth(fused, W, H).view(np.uint32), fx["depth"].view(np.uint32))
    assert (got[fx["solid_won"]] != 0).any() and (got[~fx["solid_won"]] == 0).all()
    assert stats[0] > 0 and stats[3] > 0


def test_pitched_offset_planes_give_the_same_texels_and_keep_their_padding(hip_ctx):
    fx, geo, vd, tight, stats = _fixture(hip_ctx)
    W, H = gmv.WIDTH, gmv.HEIGHT
    pitched, st = _three_ways(hip_ctx, geo, vd, W, H, "fixture, pad 5", pad=5)  # (asserts the padding of every plane, all three ways)
    for name, *_ in PLANES:
        assert pitched[name].shape[1] == (W + 5) * BPP[name] and pitched[name].shape[0] == H + 2
        assert np.array_equal(_texels(pitched, name, W, H, 5)[0], _texels(tight, name, W, H)[0]), name
    assert list(st) == list(stats)


# ---- 3: split lists that contain CUTOUT records ---------------------------------------------------------------------------------------------
def test_split_lists_with_cutout_records_equal_whole_lists_and_the_two_calls(hip_ctx, monkeypatch):
    """1500 large triangles, three in ten CUTOUT, piled on 128 x 128: every tile's list is longer than 256 entries and is cut into parts,
    which the second tile stage walks again — skipping the CUTOUT entries — and merges through tickets and cells of its own (k_split runs
    once: [5] and [6] are the G-buffer call's).  SAH_RASTER_MERGE_CAPACITY=0 (read at context creation) leaves every list whole.
    (Checked once with two deliberately wrong builds: without the CUTOUT skip this test, the tie test and the fixture test fail; with
    k_split launched a second time this one does, on the statistics.)"""
    import torch
    W = H = 128
    arrays = mesh.random_soup(31, triangles=1500, extent=1.5, size=(1.5, 4.0)).arrays()
    vd = _moved_view(W, H, position=(0.0, 0.0, 0.0)).gpu_data
    geo = _device(arrays)
    split, st = _three_ways(hip_ctx, geo, vd, W, H, "dense soup, split lists")
    assert st[5] > 0 and st[6] >= 1 and st[4] > 4 * 256
    split_two, _ = _render(hip_ctx, geo, vd, W, H, "two")
    monkeypatch.setenv("SAH_RASTER_MERGE_CAPACITY", "0")
    ctx = _new_ctx()
    try:
        whole, st_whole = _three_ways(ctx, geo, vd, W, H, "dense soup, whole lists")
        whole_two, _ = _render(ctx, geo, vd, W, H, "two")
    finally:
        torch.cuda.synchronize()
        ctx.close()
    assert st_whole[5] == 0 and list(st_whole[:5]) == list(st[:5])
    for other, what in ((whole, "fused whole"), (split_two, "two calls split"), (whole_two, "two calls whole")):
        _assert_same(split, other, f"fused split against {what}")
    # both classes won pixels: the depth differs from that of the SOLID primitives alone somewhere, and equals it somewhere
    solid = dict(arrays)
    solid["primitives"] = arrays["primitives"][arrays["primitives"]["type"] == _abi.PRIMITIVE_TYPE_SOLID]
    solid_only, _ = _render(hip_ctx, _device(solid), vd, W, H, "gbuffer")
    depth, solid_depth = _depth(split, W, H), _depth(solid_only, W, H)
    cutout_won, solid_won = depth != solid_depth, (depth == solid_depth) & (depth > 0)
    assert cutout_won.sum() > 100 and solid_won.sum() > 100, (int(cutout_won.sum()), int(solid_won.sum()))
    mv = _motion(split, W, H)
    assert (mv[cutout_won] == 0).all() and (mv[solid_won] != 0).any(-1).mean() > 0.9


# ---- 4: the two places where the motion winner is not the G-buffer winner ---------------------------------------------------------------
TRIANGLE = ((4, 4), (60, 8), (10, 58))  # pixels whose centres the vertices sit on; front-facing


def _ndc(W, H, z):
    return np.array([((2 * x + 1 - W) / W, (2 * y + 1 - H) / H, z) for x, y in TRIANGLE], np.float32)


def _tie_mesh(W, H, cutout_alpha, solid=True, cutout=True):
    """a SOLID primitive (red) and, drawn after it, a CUTOUT one (green, threshold 1/2) over the same three vertices at depth 1/2"""
    m = mesh.Mesh()
    red, green = m.add_material(mesh.material(base=(1.0, 0.1, 0.1, 1.0))), m.add_material(mesh.material(base=(0.1, 1.0, 0.1, 1.0), opacity_threshold=0.5))
    normals = [(0, 0, -1)] * 3
    if solid:
        m.add_primitive(_ndc(W, H, 0.5), normals, (0, 1, 2), red, colors=np.full(3, 0xffffffff, np.uint32))
    if cutout:
        m.add_primitive(_ndc(W, H, 0.5), normals, (0, 1, 2), green, ptype=_abi.PRIMITIVE_TYPE_CUTOUT,
                        colors=np.full(3, (cutout_alpha << 24) | 0xffffff, np.uint32))
    return m


@pytest.mark.parametrize("alpha_passes", [True, False])
def test_cutout_fragment_wins_the_tie_and_the_solid_one_gives_the_motion_vector(hip_ctx, alpha_passes):
    W = H = 64
    vd = rt.identity_view(W, H, rt.MOTION_SHIFT)
    alpha = 0xff if alpha_passes else 0x20
    both, st = _three_ways(hip_ctx, _device(_tie_mesh(W, H, alpha).arrays()), vd, W, H, f"SOLID + CUTOUT tie, alpha {alpha}")
    assert st[3] == 2  # both primitives are in the shared records and bin lists
    solid_only, _ = _render(hip_ctx, _device(_tie_mesh(W, H, alpha, cutout=False).arrays()), vd, W, H, "two")
    cutout_only, _ = _render(hip_ctx, _device(_tie_mesh(W, H, alpha, solid=False).arrays()), vd, W, H, "gbuffer")
    covered = _depth(both, W, H) > 0
    assert covered.sum() > 1000 and np.array_equal(covered, _depth(solid_only, W, H) > 0)
    colour = _texels(both, "color", W, H)[0]
    winner = cutout_only if alpha_passes else solid_only
    assert np.array_equal(colour, _texels(winner, "color", W, H)[0]), "the colour is not the expected primitive's"
    green_wins = colour[..., 1][covered].astype(int) > colour[..., 0][covered].astype(int)
    assert green_wins.all() if alpha_passes else not green_wins.any()
    # the motion vector is the SOLID primitive's either way: non-zero on every covered pixel, about MOTION_SHIFT
    mv = _motion(both, W, H)
    assert np.array_equal(mv, _motion(solid_only, W, H))
    assert (mv[covered] != 0).all() and (mv[~covered] == 0).all()
    assert np.abs(mv.view(np.float16).astype(np.float64)[covered] - np.array(rt.MOTION_SHIFT)).max() < 0.05


def test_solid_triangle_at_depth_zero_keeps_the_quirk_of_the_two_calls(hip_ctx):
    """clip z = 0 exactly: the G-buffer test z > 0 drops every fragment (all planes hold clear values), the motion pass's EQUAL test
    against the cleared depth accepts them.  Whatever sah_motion_vectors_render writes there, the fused call writes too."""
    W = H = 64
    m = mesh.Mesh()
    m.add_primitive(_ndc(W, H, 0.0), [(0, 0, -1)] * 3, (0, 1, 2), m.add_material(mesh.material()), colors=np.full(3, 0xffffffff, np.uint32))
    fused, st = _three_ways(hip_ctx, _device(m.arrays()), rt.identity_view(W, H, rt.MOTION_SHIFT), W, H, "SOLID triangle at z = 0")
    assert st[3] == 1
    assert (fused["depth"] == 0).all() and (fused["color"] == 0).all() and (fused["data"] == 0).all() and (fused["emission"] == 0).all()
    normals = np.ascontiguousarray(_texels(fused, "normals", W, H)[0]).view(np.uint16)
    assert (normals == np.array([0x3800, 0x3800, 0x3c00, 0], np.uint16)).all()
    print(f"z = 0: {int((_motion(fused, W, H) != 0).any(-1).sum())} texels of the motion plane are written over a cleared depth")


# ---- 5: the repeated pass -------------------------------------------------------------------------------------------------------------------
def test_repeated_fused_pass_equals_the_two_calls_and_leaves_nothing_stale(hip_ctx, fresh_ctx):
    import torch
    W, H = 250, 500
    block, offsets = ex.instanced(W, H, 7, (4, 8), "instanced-s7", mixed_winding=True)
    geo = _device(ex.to_mesh(block, offsets).arrays())
    vd = rt.identity_view(W, H, rt.MOTION_SHIFT)
    assert fresh_ctx.raster_last_pass()["attempts"] == 0
    fused, st = _render(fresh_ctx, geo, vd, W, H, "fused")
    one = fresh_ctx.raster_last_pass()
    print(f"fused, 81 draws of 64 triangles: {one}")
    assert one["attempts"] >= 2 and one["record_capacity"] >= 5184 == st[0]
    other = _new_ctx()
    try:
        two, st_two = _render(other, geo, vd, W, H, "two")
    finally:
        torch.cuda.synchronize()
        other.close()
    _assert_same(fused, two, "repeated fused pass against the two calls on a context of their own")
    assert list(st[:5]) == list(st_two[:5])
    again, st_again = _render(fresh_ctx, geo, vd, W, H, "fused")
    assert fresh_ctx.raster_last_pass()["attempts"] == 1
    _assert_same(fused, again, "second fused call against the first")
    # the small fixture scene on the grown context
    fx, fgeo, fvd, want, want_stats = _fixture(hip_ctx)
    small, st_small = _render(fresh_ctx, fgeo, fvd, gmv.WIDTH, gmv.HEIGHT, "fused")
    assert fresh_ctx.raster_last_pass()["attempts"] == 1 and fresh_ctx.raster_last_pass()["record_capacity"] >= 5184
    _assert_same(small, want, "fixture on the grown context")
    assert list(st_small) == list(want_stats)


# ---- 6: near-plane clipping -----------------------------------------------------------------------------------------------------------------
def test_clipped_fans_are_found_through_the_sequence_table(hip_ctx):
    W, H = 160, 90
    vd = _moved_view(W, H, position=(0.0, 1.0, 0.0)).gpu_data  # inside the atrium: its floor and walls cross the near plane
    fused, st = _three_ways(hip_ctx, _device(mesh.atrium(8).arrays()), vd, W, H, "atrium from inside")
    assert st[0] == 23808 and st[3] > st[0] - st[1] - st[2], "no triangle of this frame was clipped into a fan"
    solid = _depth(fused, W, H) > 0  # every primitive of the atrium is SOLID
    mv = _motion(fused, W, H)
    assert solid.mean() > 0.5 and (mv[~solid] == 0).all() and (mv[solid] != 0).any(-1).mean() > 0.9


# ---- 7: no side effects ---------------------------------------------------------------------------------------------------------------------
def test_no_side_effects_on_shadow_rsm_epoch_and_the_standalone_passes(hip_ctx):
    import torch
    W, H = 320, 180
    view = _moved_view(W, H)
    arrays = mesh.random_soup(41, triangles=800, extent=8.0).arrays()
    geo = _device(arrays)
    _, sun, lpv = _setup(W, H)
    sun.update_shadow_cascades(view, resolution=256)

    def shadow():
        sm = torch.full((4, 256, 256), 7, dtype=torch.int16, device="cuda")
        with _limit():
            hip_ctx.shadow_render(geo, sun.constants, 4, images.volume(sm, _abi.FORMAT_D16_UNORM))
            torch.cuda.synchronize()
        return sm

    def rsm():
        with _limit():
            out = _hip_rsm(hip_ctx, arrays, sun, lpv)
            torch.cuda.synchronize()
        return out
    two_before, _ = _render(hip_ctx, geo, view.gpu_data, W, H, "two")
    sm0, rsm0 = shadow(), rsm()
    epoch = hip_ctx.cache_epoch()
    fused, _ = _render(hip_ctx, geo, view.gpu_data, W, H, "fused")
    assert hip_ctx.cache_epoch() == epoch
    # the stand-alone passes right after it, on the scratch it left: the motion pass first (against the fused call's depth bytes)
    two_after, _ = _render(hip_ctx, geo, view.gpu_data, W, H, "two")
    sm1 = shadow()
    fused_again, _ = _render(hip_ctx, geo, view.gpu_data, W, H, "fused")
    rsm1 = rsm()
    assert hip_ctx.cache_epoch() == epoch
    assert torch.equal(sm0, sm1) and all(torch.equal(rsm0[k], rsm1[k]) for k in rsm0)
    _assert_same(two_before, two_after, "the two calls after the fused call against before it")
    _assert_same(fused, two_before, "the fused call against the two calls")
    _assert_same(fused, fused_again, "the fused call between the other rasteriser passes")
    assert (_motion(fused, W, H) != 0).any()


# ---- 8: an empty scene ----------------------------------------------------------------------------------------------------------------------
def test_empty_scene_clears_every_plane(hip_ctx):
    W, H = 70, 66  # two tiles each way, the second ones partial
    fused, st = _three_ways(hip_ctx, _abi.SceneGeometry(), rt.identity_view(W, H, rt.MOTION_SHIFT), W, H, "empty scene")
    assert not st.any()
    for name in ("color", "data", "emission", "depth", "motion_vectors"):
        assert (fused[name] == 0).all(), name
    assert (np.ascontiguousarray(_texels(fused, "normals", W, H)[0]).view(np.uint16) == np.array([0x3800, 0x3800, 0x3c00, 0], np.uint16)).all()
