"""The repeated pass of the rasteriser, observed (sah_debug_raster_last_pass).

run() in api_raster.cpp sizes its scratch from guesses, launches both stages, reads the counters back and, where a buffer was too small, grows
it and renders the pass AGAIN: the first attempt relies on every guard of the kernels that keeps a short buffer from being overrun (records,
attributes, clip queue, bin lists, sequence table, extra list parts), the second on nothing stale surviving the first (tickets, merge
buffers, tile cursors, split slots).  Instanced index ranges are enough to get there: the record guess counts index triples, not draws.

Every case runs on a context of its own, because the scratch only grows; the first call must take two attempts or more, an identical second
call one, and the images and statistics words 0-3 of both must equal each other and the oracle.  The sizes follow the code's own formulas:
ensure() allocates bytes * 1.25 + 256, and the guesses are
    records   want = (num_indices / 3) * views + 1024                      (56-byte records; one attribute record each: 160 / 96 / 84 bytes)
    clip      want = records / 8 + 1024                                    (8-byte entries)
    bin lists want = max(the last call's, 2 * records + 4 * tiles)         (4-byte entries)
    sequence  want = max(the last call's, (num_indices / 3) * 8 * views + 64)   (not for the shadow pass)"""
import numpy as np
import pytest

from androidrenderer_amd import _abi, lib, mesh
from tests import raster_exact_ref as ex
from tests import raster_ties_util as rt
from tests import test_raster_ties_gpu as tg

pytestmark = pytest.mark.gpu

RECORD_BYTES = 56


def _capacity(want, item_bytes):
    """entries of a buffer that ensure() sized for `want` entries"""
    b = want * item_bytes
    return (b + b // 4 + 256) // item_bytes


@pytest.fixture
def fresh_ctx():
    import torch
    ctx = lib.Context(device=0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    yield ctx
    torch.cuda.synchronize()
    ctx.close()


# ---- records and sequence table: a 64-triangle primitive drawn 81 times -----------------------------------------------------------------
# num_indices / 3 = 64, so the record guess is 64 * views + 1024 = 1088 (one view) or 1280 (four): capacities 1364 and 1604 at most, against
# 5184 * views records needed; the sequence table is guessed at 64 * 8 * views + 64 = 576 entries (capacity 784) against 41473 needed.
W, H = 250, 500


def _instanced(solid=False):
    block, offsets = ex.instanced(W, H, 7, (4, 8), "instanced-s7", mixed_winding=not solid)
    if solid:
        block = block.as_class(ex.SOLID)
    assert len(block.tri) == 64 and len(offsets) == 81
    return block, offsets, ex.flatten(block, offsets)


def _twice(ctx, render, views, needed_records, what):
    """render() on a fresh context and again; returns (first, second) results after the assertions on the hook"""
    assert ctx.raster_last_pass()["attempts"] == 0
    first = render()
    one = ctx.raster_last_pass()
    second = render()
    two = ctx.raster_last_pass()
    print(f"{what}: first call {one}, second call {two}")
    assert one["attempts"] >= 2, f"{what}: the first call was not repeated: {one}"
    assert two["attempts"] == 1 and {k: two[k] for k in two if k != "attempts"} == {k: one[k] for k in one if k != "attempts"}
    if needed_records is not None:
        assert _capacity(64 * views + 1024, RECORD_BYTES) < needed_records <= one["record_capacity"]
    return first, second


def _equal(a, b, what):
    if isinstance(a, dict):
        for k in a:
            tg._same(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k], f"{what} '{k}'")
    else:
        tg._same(a, b, what)


def test_gbuffer_pass_is_repeated_for_instanced_draws(fresh_ctx):
    block, offsets, flat = _instanced()
    arrays = ex.to_mesh(block, offsets).arrays()
    geo = tg._device_geometry(arrays)
    (got1, st1), (got2, st2) = _twice(fresh_ctx, lambda: tg.hip_gbuffer(fresh_ctx, geo, W, H), 1, 5184, "G-buffer, 81 draws of 64 triangles")
    want, want_stats = rt.oracle_gbuffer_of(arrays, W, H)
    _equal(got1, got2, "G-buffer, second call against the first")
    _equal(got1, want, "G-buffer against the oracle")
    assert list(st1[:4]) == list(st2[:4]) == list(want_stats[:4]) and st1[0] == 5184
    cov = ex.coverage(flat)
    owner, depth_n = ex.owners(flat, cov, "gbuffer")
    assert (cov.count == 1).all()
    tg._same(got1["depth"].view(np.uint32), ex.depth_bits(depth_n), "G-buffer depth against the exact reference")
    rt.assert_owner(got1["color"], flat, owner, "G-buffer colour")


def test_shadow_pass_is_repeated_for_instanced_draws(fresh_ctx):
    import ctypes as C
    from androidrenderer_amd import images
    from tests import util
    block, offsets, flat = _instanced()
    arrays = ex.to_mesh(block, offsets).arrays()
    geo = tg._device_geometry(arrays)
    (got1, st1), (got2, st2) = _twice(fresh_ctx, lambda: tg.hip_shadow(fresh_ctx, geo, 4, W, H), 4, 4 * 5184, "shadow, 4 cascades, 81 draws of 64 triangles")
    want, want_stats = np.zeros((4, H, W), np.uint16), np.zeros(_abi.RASTER_STATS_WORDS, np.uint32)
    vol = images.volume(want, _abi.FORMAT_D16_UNORM)
    assert util.oracle().orc_shadow_render(C.byref(rt.host_geometry(arrays)), C.byref(rt.identity_sun()), 4, C.byref(vol), want_stats.ctypes.data) == 0
    _equal(got1, got2, "shadow cascades, second call against the first")
    _equal(got1, want, "shadow cascades against the oracle")
    assert list(st1[:4]) == list(st2[:4]) == list(want_stats[:4])
    _, depth_n = ex.owners(flat, ex.coverage(flat), "shadow")
    for layer in range(4):
        tg._same(got1[layer].astype(np.int64), ex.d16_code(depth_n), f"shadow cascade {layer} against the exact reference")


def test_rsm_pass_is_repeated_for_instanced_draws(fresh_ctx):
    import ctypes as C
    from tests import util
    block, offsets, flat = _instanced()
    arrays = ex.to_mesh(block, offsets).arrays()
    geo = tg._device_geometry(arrays)
    (got1, st1), (got2, st2) = _twice(fresh_ctx, lambda: tg.hip_rsm(fresh_ctx, geo, 2, W, H), 2, 2 * 5184, "RSM, 2 cascades, 81 draws of 64 triangles")
    want, want_stats = rt.new_rsm(2, W, H), np.zeros(_abi.RASTER_STATS_WORDS, np.uint32)
    d = rt.rsm_targets(want)
    assert util.oracle().orc_rsm_render(C.byref(rt.host_geometry(arrays)), C.byref(rt.identity_sun()), rt.identity_lpv(), 2, C.byref(d), want_stats.ctypes.data) == 0
    _equal(got1, got2, "RSM, second call against the first")
    _equal(got1, want, "RSM against the oracle")
    assert list(st1[:4]) == list(st2[:4]) == list(want_stats[:4])
    owner, depth_n = ex.owners(flat, ex.coverage(flat), "rsm")
    for layer in range(2):
        tg._same(got1["depth"][layer].astype(np.int64), ex.d16_code(depth_n), f"RSM depth layer {layer} against the exact reference")
        rt.assert_owner(got1["flux"][layer], flat, owner, f"RSM flux layer {layer}")


def test_motion_pass_is_repeated_for_instanced_draws(fresh_ctx):
    """the depth plane comes from the exact reference (a G-buffer call on this context would grow the records first)"""
    import torch
    block, offsets, flat = _instanced(solid=True)
    geo = tg._device_geometry(ex.to_mesh(block, offsets).arrays())
    cov = ex.coverage(flat)
    owner, depth_n = ex.owners(flat, cov, "gbuffer")
    assert (cov.count == 1).all()
    depth = torch.from_numpy(ex.depth_bits(depth_n).view(np.float32).copy()).cuda()
    depth[::2, ::3] = 0.8751  # no fragment has this depth (depths are multiples of 1/64): those pixels keep the clear value
    wins = np.ones((H, W), bool)
    wins[::2, ::3] = False
    (got1, st1), (got2, st2) = _twice(fresh_ctx, lambda: tg.hip_motion(fresh_ctx, geo, depth, W, H), 1, 5184, "motion vectors, 81 draws of 64 triangles")
    want = rt.motion_vectors_fp32(flat, owner, wins, rt.MOTION_SHIFT, rt.instanced_world(block, offsets))
    _equal(got1, got2, "motion vectors, second call against the first")
    _equal(got1, want, "motion vectors against the fp32 restatement")
    tg._same((got1 != 0).any(-1), wins, "motion vectors: non-zero exactly where the owner's depth is the depth texel")
    assert list(st1[:4]) == list(st2[:4]) == [5184, 0, 0, 5184]


# ---- clip queue and appended fans: 3000 long triangles that all cross the near plane ----------------------------------------------------
# records are guessed at 3000 + 1024 = 4024 (capacity 5034) and the clip queue at 4024 / 8 + 1024 = 1527 entries (capacity 1940): the first
# attempt queues 1940 of the 3000, appends their fans (two triangles each) behind the 3000 direct slots until the records run out as
# well, and the second is sized for 3000 + the appended + 7 per queued triangle.
def _near_plane_mesh(n=3000, seed=17):
    g = np.random.default_rng(seed)
    ang = g.uniform(0, 2 * np.pi, n)
    c = g.uniform(-0.95, 0.95, (n, 2))
    d = np.stack([np.cos(ang), np.sin(ang)], -1)
    length, half = g.uniform(0.1, 0.5, (n, 1)), g.uniform(0.01, 0.03, (n, 1))
    nrm = np.stack([-d[:, 1], d[:, 0]], -1)
    tip, a, b = c - length * d, c + length * d + half * nrm, c + length * d - half * nrm
    z = np.stack([np.full(n, -0.25), g.integers(8, 60, n) / 64.0, g.integers(8, 60, n) / 64.0], -1)  # the tip lies behind the plane z = 0
    pos = np.concatenate([np.stack([tip, a, b], 1), z[..., None]], -1).reshape(-1, 3).astype(np.float32)
    m = mesh.Mesh()
    mats = [m.add_material(mesh.material(base=(r, gr, b_, 1.0))) for (r, gr, b_) in ((1, 0.5, 0.25), (0.25, 1, 0.5))]
    colours = g.integers(0, 1 << 24, 3 * n, dtype=np.uint64).astype(np.uint32) | np.uint32(0xff000000)
    half_n = 3 * (n // 2)
    m.add_primitive(pos[:half_n], [(0, 0, -1)] * half_n, np.arange(half_n), mats[0], ptype=_abi.PRIMITIVE_TYPE_CUTOUT, colors=colours[:half_n])
    m.add_primitive(pos[half_n:], [(0, 0, -1)] * (3 * n - half_n), np.arange(3 * n - half_n), mats[1], ptype=_abi.PRIMITIVE_TYPE_CUTOUT, colors=colours[half_n:])
    return m


def test_gbuffer_pass_is_repeated_for_a_short_clip_queue(fresh_ctx):
    w, h, n = 200, 136, 3000
    arrays = _near_plane_mesh(n).arrays()
    geo = tg._device_geometry(arrays)
    (got1, st1), (got2, st2) = _twice(fresh_ctx, lambda: tg.hip_gbuffer(fresh_ctx, geo, w, h), 1, None, "G-buffer, 3000 triangles across the near plane")
    one = fresh_ctx.raster_last_pass()
    assert _capacity((n + 1024) // 8 + 1024, 8) < n <= one["clip_capacity"]
    want, want_stats = rt.oracle_gbuffer_of(arrays, w, h)
    _equal(got1, got2, "G-buffer, second call against the first")
    _equal(got1, want, "G-buffer against the oracle")
    assert list(st1[:4]) == list(st2[:4]) == list(want_stats[:4])
    assert st1[0] == n and st1[3] > n and one["record_capacity"] >= n + st1[3], "every triangle is clipped into a fan of two"
    assert (want["depth"] > 0).mean() > 0.3


# ---- bin lists: 600 triangles that span a 512 x 512 image (64 tiles) ---------------------------------------------------------------------
# the bin lists are guessed at 2 * (600 + 1024) + 4 * 64 = 3504 entries (capacity 4444); 600 slivers from border to border through the
# middle of the image have boxes of 16 tiles and more (binned through tile_outside) and leave about 10000 entries, several hundred of
# them in each of the four tiles around the centre (lists that are cut into parts — in the first, short attempt too).
def _star_mesh(n=600, seed=9):
    g = np.random.default_rng(seed)
    ang = g.uniform(0, np.pi, n)
    c = g.uniform(-0.08, 0.08, (n, 2))
    d = np.stack([np.cos(ang), np.sin(ang)], -1)
    nrm = np.stack([-d[:, 1], d[:, 0]], -1)
    half = g.uniform(0.004, 0.02, (n, 1))
    v = np.stack([c - 1.6 * d, c + 1.6 * d + half * nrm, c + 1.6 * d - half * nrm], 1)
    z = np.repeat(g.integers(1, 64, (n, 1)) / 64.0, 3, axis=1)
    pos = np.concatenate([v, z[..., None]], -1).reshape(-1, 3).astype(np.float32)
    m = mesh.Mesh()
    mat = m.add_material(mesh.material())
    colours = g.integers(0, 1 << 24, 3 * n, dtype=np.uint64).astype(np.uint32) | np.uint32(0xff000000)
    m.add_primitive(pos, [(0, 0, -1)] * (3 * n), np.arange(3 * n), mat, ptype=_abi.PRIMITIVE_TYPE_CUTOUT, colors=colours)
    return m


def test_gbuffer_pass_is_repeated_for_short_bin_lists(fresh_ctx):
    w = h = 512
    n = 600
    arrays = _star_mesh(n).arrays()
    geo = tg._device_geometry(arrays)
    (got1, st1), (got2, st2) = _twice(fresh_ctx, lambda: tg.hip_gbuffer(fresh_ctx, geo, w, h), 1, None, "G-buffer, 600 slivers across 64 tiles")
    one = fresh_ctx.raster_last_pass()
    assert _capacity(2 * (n + 1024) + 4 * 64, 4) < st1[4] <= one["pairs_capacity"], f"{st1[4]} bin entries"
    assert one["record_capacity"] == _capacity(n + 1024, 160), "the records and the clip queue of this case were large enough from the start"
    assert st1[5] > 0 and st1[6] >= 1, "the lists of the tiles around the centre are cut into parts"
    want, want_stats = rt.oracle_gbuffer_of(arrays, w, h)
    _equal(got1, got2, "G-buffer, second call against the first")
    _equal(got1, want, "G-buffer against the oracle")
    assert list(st1[:5]) == list(st2[:5]) and list(st1[:4]) == list(want_stats[:4])


# ---- growth within one context ------------------------------------------------------------------------------------------------------------
def test_small_scene_after_a_large_one_reads_nothing_stale(fresh_ctx):
    """small scene, the instanced one (which grows every buffer), the near-plane one (which appends fans and fills the sequence table), the
    small scene again: it gives its first result — records, attributes and sequence slots beyond the new counts are not read — in one
    attempt, through buffers that kept their size"""
    small = tg._device_geometry(rt.mesh_of("jitter-s40", "z").arrays())
    sc = rt.scene_of("jitter-s40", "z")
    block, offsets, _ = _instanced()
    large = tg._device_geometry(ex.to_mesh(block, offsets).arrays())
    clipped = tg._device_geometry(_near_plane_mesh().arrays())

    def render_small():
        out = (tg.hip_gbuffer(fresh_ctx, small, sc.W, sc.H), tg.hip_shadow(fresh_ctx, small, 4, sc.W, sc.H), tg.hip_rsm(fresh_ctx, small, 2, sc.W, sc.H))
        return out, fresh_ctx.raster_last_pass()

    before, hook_before = render_small()
    assert hook_before["attempts"] == 1
    tg.hip_gbuffer(fresh_ctx, large, W, H)
    assert fresh_ctx.raster_last_pass()["attempts"] >= 2
    tg.hip_shadow(fresh_ctx, large, 4, W, H)
    assert fresh_ctx.raster_last_pass()["attempts"] >= 2
    tg.hip_rsm(fresh_ctx, large, 2, W, H)
    tg.hip_gbuffer(fresh_ctx, clipped, 200, 136)
    grown = fresh_ctx.raster_last_pass()
    after, hook_after = render_small()
    assert hook_after["attempts"] == 1 and hook_after["record_capacity"] >= 4 * 5184 > hook_before["record_capacity"]  # (the near-plane scene asked for 27880)
    assert hook_after["clip_capacity"] == grown["clip_capacity"] and hook_after["pairs_capacity"] >= grown["pairs_capacity"]
    for (a, sa), (b, sb), what in zip(before, after, ("G-buffer", "shadow cascades", "RSM")):
        _equal(a, b, f"{what} of the small scene after the large ones")
        assert list(sa[:5]) == list(sb[:5])
    _, _, own = rt.exact("jitter-s40", "z")
    tg._same(after[0][0]["depth"].view(np.uint32), ex.depth_bits(own["gbuffer"][1]), "G-buffer depth of the small scene against the exact reference")
    tg._same(after[1][0][0].astype(np.int64), ex.d16_code(own["rsm"][1]), "shadow cascade 0 of the small scene against the exact reference")
