"""What tests/test_raster_ties_cpu.py and tests/test_raster_ties_gpu.py share: the cases of tests/raster_exact_ref.py with their exact
results (computed once per process), the oracle's images of them, the identity views, the owner read-out and the fp32 restatement of the
motion vectors of such a scene."""
import ctypes as C
import functools

import numpy as np

from androidrenderer_amd import _abi, images, mesh
from tests import raster_exact_ref as ex
from tests import util

CASES = ex.cases()
NAMES = sorted(CASES)
ORDERS = ("z", "1-z")
SAME_DEPTH_CASE = "jitter-s13"  # rendered once more as two copies at one depth: draw order alone decides
MOTION_SHIFT = (3, -2)          # whole pixels between the last frame's projection and this one's


def identity16():
    return (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))


def identity_view(W, H, shift=(0, 0)):
    """sah_view_data with identity view and projection; last_frame_projection translates by `shift` whole pixels"""
    v = _abi.ViewData()
    for name in ("view", "projection", "inverse_view", "inverse_projection", "last_frame_view", "last_frame_projection"):
        setattr(v, name, identity16())
    v.last_frame_projection[12], v.last_frame_projection[13] = 2.0 * shift[0] / W, 2.0 * shift[1] / H  # column-major: the translation column
    v.render_resolution[0], v.render_resolution[1] = W, H
    return v


def identity_sun(num_cascades=4):
    sun = _abi.SunLightConstants()
    for c in range(num_cascades):
        for i in range(4):
            sun.cascade_matrices[c][i * 5] = 1.0
    sun.direction_and_tan_size[2] = 1.0  # light along +z onto normals (0, 0, -1)
    for k in range(3):
        sun.color[k] = 1.0
    return sun


def identity_lpv(num_cascades=4):
    m = (_abi.LpvCascadeMatrices * num_cascades)()
    for c in range(num_cascades):
        m[c].rsm_vp = identity16()
    return m


def scene_of(name, order):
    """the Scene of a case; order 'z' or '1-z'; name 'same-depth': SAME_DEPTH_CASE twice at depth 1/2, the second copy under other ids"""
    if name == "same-depth":
        one = CASES[SAME_DEPTH_CASE].with_depth(32)
        two = ex.Scene(one.name, one.W, one.H, one.tri, one.depth_n, one.cls, one.ids + 171)
        return one.joined(two)
    return CASES[name] if order == "z" else CASES[name].flipped()


def mesh_of(name, order):
    sc = scene_of(name, order)
    return ex.to_mesh(sc) if name == "same-depth" else ex.case_mesh(name, sc)


@functools.lru_cache(maxsize=None)
def exact(name, order):
    """(scene, coverage, {rule: (owner, depth_n)}) of a case, computed once"""
    sc = scene_of(name, order)
    cov = ex.coverage(sc)
    return sc, cov, {rule: ex.owners(sc, cov, rule) for rule in ("gbuffer", "rsm")}


def new_gbuffer(W, H, pad=0):
    return {"color": np.zeros((H, W + pad, 4), np.uint8), "normals": np.zeros((H, W + pad, 4), np.uint16), "data": np.zeros((H, W + pad, 4), np.uint8),
            "emission": np.zeros((H, W + pad, 4), np.uint8), "depth": np.zeros((H, W + pad), np.float32)}


def host_geometry(arrays):
    return mesh.geometry(mesh.with_counts(arrays), [])


@functools.lru_cache(maxsize=None)
def oracle_shadow(name, order, cascades):
    sc = scene_of(name, order)
    sm = np.zeros((cascades, sc.H, sc.W), np.uint16)
    stats = np.zeros(_abi.RASTER_STATS_WORDS, np.uint32)
    vol = images.volume(sm, _abi.FORMAT_D16_UNORM)
    assert util.oracle().orc_shadow_render(C.byref(host_geometry(mesh_of(name, order).arrays())), C.byref(identity_sun()), cascades, C.byref(vol), stats.ctypes.data) == 0
    return sm, stats


def oracle_gbuffer_of(arrays, W, H):
    out = new_gbuffer(W, H)
    stats = np.zeros(_abi.RASTER_STATS_WORDS, np.uint32)
    gb = images.gbuffer(out)
    assert util.oracle().orc_gbuffer_render(C.byref(host_geometry(arrays)), C.byref(identity_view(W, H)), C.byref(gb), stats.ctypes.data) == 0
    return out, stats


@functools.lru_cache(maxsize=None)
def oracle_gbuffer(name, order):
    sc = scene_of(name, order)
    return oracle_gbuffer_of(mesh_of(name, order).arrays(), sc.W, sc.H)


def new_rsm(cascades, W, H):
    return {"flux": np.zeros((cascades, H, W, 4), np.uint8), "normals": np.zeros((cascades, H, W, 4), np.uint8), "depth": np.zeros((cascades, H, W), np.uint16)}


def rsm_targets(t):
    return _abi.RsmTargets(images.volume(t["flux"], _abi.FORMAT_R8G8B8A8_SRGB), images.volume(t["normals"], _abi.FORMAT_R8G8B8A8_UNORM),
                           images.volume(t["depth"], _abi.FORMAT_D16_UNORM))


@functools.lru_cache(maxsize=None)
def oracle_rsm(name, order, cascades=1):
    sc = scene_of(name, order)
    out = new_rsm(cascades, sc.W, sc.H)
    stats = np.zeros(_abi.RASTER_STATS_WORDS, np.uint32)
    d = rsm_targets(out)
    assert util.oracle().orc_rsm_render(C.byref(host_geometry(mesh_of(name, order).arrays())), C.byref(identity_sun()), identity_lpv(), cascades, C.byref(d),
                                        stats.ctypes.data) == 0
    return out, stats


def assert_owner(rgb, scene, owner, what):
    """The colour plane `rgb` (H, W, >= 3) shows, pixel by pixel, the triangle `owner` says: a triangle's vertex colour carries its id as
    one of 8 levels per channel (31, 63 .. 255 of 255), and whatever a pass makes of a level — the G-buffer's sRGB code of the half colour,
    the RSM's flux — is one code (give or take the half rounding of the interpolation: 2 codes) per level and grows with the level, the
    codes of two levels far apart.  So the plane names the owner without the test knowing the transfer function."""
    covered = owner >= 0
    assert covered.all(), f"{what}: the exact reference leaves pixels uncovered"
    levels = ex.id_levels(scene.ids[owner])
    for ch in range(3):
        last_hi = -100
        for level in range(ex.LEVELS):
            codes = rgb[..., ch][levels[..., ch] == level].astype(np.int64)
            if not codes.size:
                continue
            lo, hi = int(codes.min()), int(codes.max())
            assert hi - lo <= 2, f"{what}: channel {ch}, level {level}: codes {lo} .. {hi} — some pixel shows another triangle than its owner"
            assert lo >= last_hi + 8, f"{what}: channel {ch}, level {level}: codes from {lo} on overlap the level below (up to {last_hi})"
            last_hi = hi


# ---- motion vectors of such a scene, restated in fp32 ------------------------------------------------------------------------------------
f32 = np.float32


def motion_scene(name, order):
    """the case as CUTOUT triangles and, listed after them, once more as SOLID front faces at the depths of the OTHER order: the motion pass
    draws the SOLID copy alone and keeps a pixel where the SOLID owner's depth is the G-buffer's, i.e. where it is not behind the CUTOUT one"""
    cut = scene_of(name, order)
    front = ex.Scene(cut.name, cut.W, cut.H, _front_facing(cut.tri), 64 - cut.depth_n, np.full(len(cut.tri), ex.SOLID), cut.ids + 77)
    return cut.joined(front)


def _front_facing(tri):
    t = tri.copy()
    area = (t[:, 1, 0] - t[:, 0, 0]) * (t[:, 2, 1] - t[:, 0, 1]) - (t[:, 2, 0] - t[:, 0, 0]) * (t[:, 1, 1] - t[:, 0, 1])
    back = area < 0
    t[back, 1], t[back, 2] = tri[back, 2], tri[back, 1]
    return t


def motion_mesh(name, order):
    return ex.to_mesh(motion_scene(name, order))


@functools.lru_cache(maxsize=None)
def motion_exact(name, order):
    """(scene, solid_wins (H, W) bool, expected (H, W, 2) uint16, depth_n (H, W) of the G-buffer): where the exact reference says the SOLID owner's depth equals the G-buffer's
    depth, and the vector the pass's fp32 arithmetic (raster_tiles.hip: motion_vector_of; tools/gen_golden_motion_vectors.py) gives there"""
    sc = motion_scene(name, order)
    cov = ex.coverage(sc)
    _, depth_all = ex.owners(sc, cov, "gbuffer")
    frag = sc.cls[cov.frag_tri] == ex.SOLID
    cov_s = ex.Coverage()
    cov_s.frag_pix, cov_s.frag_tri = cov.frag_pix[frag], cov.frag_tri[frag]
    owner_s, depth_s = ex.owners(sc, cov_s, "gbuffer")
    wins = (owner_s >= 0) & (depth_s == depth_all)
    return sc, wins, motion_vectors_fp32(sc, owner_s, wins, MOTION_SHIFT), depth_all


def instanced_world(block, offsets):
    """fp32 world x, y (T, 3) of the triangles of ex.flatten(block, offsets) as the vertex stage computes them: the block's stored position plus
    the translation of the draw's model matrix, one fp32 addition"""
    W, H = block.W, block.H
    bx, by = ((2 * block.tri[..., 0] + 1 - W) / W).astype(f32), ((2 * block.tri[..., 1] + 1 - H) / H).astype(f32)
    return (np.concatenate([bx + f32(2.0 * dx / W) for dx, _ in offsets]), np.concatenate([by + f32(2.0 * dy / H) for _, dy in offsets]))


def motion_vectors_fp32(sc, owner, wins, shift, world=None):
    """fp32, operator by operator, for triangles with w = 1 under identity matrices: screen-space barycentrics b_i = (float)E_i * (1 / (float)area),
    perspective weights l_i = b_i / ((b_0 + b_1) + b_2), the last frame's clip position interpolated, divided, turned into pixels, minus the
    pixel centre, rounded to half"""
    W, H = sc.W, sc.H
    t = np.maximum(owner, 0)
    X, Y = sc.tri[t][..., 0] * 256 + 128, sc.tri[t][..., 1] * 256 + 128  # (H, W, 3)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    cx, cy = xs * 256 + 128, ys * 256 + 128
    area = (X[..., 1] - X[..., 0]) * (Y[..., 2] - Y[..., 0]) - (X[..., 2] - X[..., 0]) * (Y[..., 1] - Y[..., 0])
    inv_area = f32(1) / np.where(wins, area, 1).astype(f32)
    b = []
    for i in range(3):
        a_, b_ = (i + 1) % 3, (i + 2) % 3
        e = (X[..., b_] - X[..., a_]) * (cy - Y[..., a_]) - (Y[..., b_] - Y[..., a_]) * (cx - X[..., a_])
        b.append(e.astype(f32) * inv_area)
    s = (b[0] + b[1]) + b[2]
    with np.errstate(all="ignore"):
        lam = [bi / s for bi in b]
    # vertex stage: NDC position as the mesh stores it (ex.add_to_mesh), then model, last_frame_view (identity), last_frame_projection (a translation)
    if world is None:
        world = (((2 * sc.tri[..., 0] + 1 - W) / W).astype(f32), ((2 * sc.tri[..., 1] + 1 - H) / H).astype(f32))
    px, py = world[0][t], world[1][t]
    tx, ty = f32(2.0 * shift[0] / W), f32(2.0 * shift[1] / H)
    prev = (px + tx * f32(1), py + ty * f32(1), np.ones_like(px))  # ((1 x + 0 y) + 0 z) + t w: the zero terms change nothing
    centre = ((xs.astype(f32) + f32(0.5)), (ys.astype(f32) + f32(0.5)))
    res = (f32(W), f32(H))
    out = np.zeros((H, W, 2), np.uint16)
    with np.errstate(all="ignore"):
        v = [(lam[0] * p[..., 0] + lam[1] * p[..., 1]) + lam[2] * p[..., 2] for p in prev]
        for c in range(2):
            ndc = v[c] / v[2]
            uv = ndc * f32(0.5) + f32(0.5)
            mv = uv * res[c] - centre[c]
            out[..., c] = np.where(wins, mv.astype(np.float16).view(np.uint16), 0)
    return out
