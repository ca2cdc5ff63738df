"""Edges through pixel centres, on the CPU: the scenes of tests/raster_exact_ref.py have power (the exact reference alone says so), and the
oracle's shadow, G-buffer and RSM passes equal the exact integer reference on every one of them — coverage, depth and owner.  The GPU half
is tests/test_raster_ties_gpu.py.

Why: a triangle soup with vertices snapped to 1/256 px essentially never puts an edge through a pixel centre, so the top-left rule of
DESIGN.md §5d (`e > 0 || (e == 0 && top_left)`) could turn into `e >= 0` or `e > 0` without a soup noticing; on screen that is a
double-covered seam or a crack along every shared edge of a grid-modelled mesh."""
import numpy as np
import pytest

from tests import raster_exact_ref as ex
from tests import raster_ties_util as rt


@pytest.mark.parametrize("name", rt.NAMES)
def test_every_case_is_watertight_and_has_power(name):
    """from the exact reference alone: every pixel is covered exactly once, and each wrong rule changes at least 100 pixels"""
    sc, cov, _ = rt.exact(name, "z")
    assert (cov.count == 1).all(), f"{int((cov.count != 1).sum())} pixels are not covered exactly once"
    doubly, uncovered = int((cov.count_in >= 2).sum()), int((cov.count_out == 0).sum())
    print(f"{name}: {len(sc.tri)} triangles, {sc.W}x{sc.H}; ties in: {doubly} pixels doubly covered; ties out: {uncovered} uncovered")
    assert doubly >= 100 and uncovered >= 100


@pytest.mark.parametrize("name", ["giant-diagonal-s320", "giant-antidiagonal-s320"])
def test_giant_cases_have_tiles_that_one_tie_pixel_holds(name):
    """tile_outside() of the binning (boxes of 16 tiles or more) must keep a tile whose most favourable corner lies exactly on an edge: these
    cases have triangles that touch several tiles in that one pixel only — a strict test there would lose the pixel"""
    sc, cov, _ = rt.exact(name, "z")
    held = ex.tiles_held_by_ties(sc, cov)
    print(f"{name}: (triangle, tile x, tile y) held by tie pixels alone: {held}")
    assert len(held) >= 3


def test_depth_codes_of_the_exact_reference():
    """the integer forms of the two depth encodings against the fp32 arithmetic they stand for, for every depth a scene can hold"""
    n = np.arange(1, 64)
    z = (n / 64.0).astype(np.float32)
    assert np.array_equal(ex.depth_bits(n), z.view(np.uint32))
    assert np.array_equal(ex.d16_code(n), np.rint(z * np.float32(65535)).astype(np.int64))


@pytest.mark.parametrize("order", rt.ORDERS)
@pytest.mark.parametrize("name", rt.NAMES)
def test_oracle_shadow_equals_exact(name, order):
    sc, cov, own = rt.exact(name, order)
    sm, stats = rt.oracle_shadow(name, order, 1)
    want = ex.d16_code(own["rsm"][1])
    bad = np.argwhere(sm[0] != want)
    assert bad.size == 0, f"{len(bad)} texels differ from the exact reference, first at (y, x) = {bad[0].tolist()}"
    assert stats[0] == len(sc.tri) and stats[2] == 0


@pytest.mark.parametrize("order", rt.ORDERS)
@pytest.mark.parametrize("name", rt.NAMES)
def test_oracle_gbuffer_equals_exact(name, order):
    sc, cov, own = rt.exact(name, order)
    out, stats = rt.oracle_gbuffer(name, order)
    owner, depth_n = own["gbuffer"]
    bad = np.argwhere(out["depth"].view(np.uint32) != ex.depth_bits(depth_n))
    assert bad.size == 0, f"{len(bad)} depth texels differ from the exact reference, first at (y, x) = {bad[0].tolist()}"
    rt.assert_owner(out["color"], sc, owner, f"G-buffer colour of {sc.name}")
    assert stats[0] == len(sc.tri)


@pytest.mark.parametrize("order", rt.ORDERS)
@pytest.mark.parametrize("name", rt.NAMES)
def test_oracle_rsm_equals_exact(name, order):
    sc, cov, own = rt.exact(name, order)
    out, _ = rt.oracle_rsm(name, order)
    owner, depth_n = own["rsm"]
    assert np.array_equal(out["depth"][0], ex.d16_code(depth_n))
    rt.assert_owner(out["flux"][0], sc, owner, f"RSM flux of {sc.name}")


def test_equal_depths_are_decided_by_draw_order():
    """two copies of a case at ONE depth: the last draw stays in the G-buffer, the first in the RSM — and a fragment too many on a shared
    edge would be a later (or earlier) draw than the owner's"""
    sc, cov, own = rt.exact("same-depth", "z")
    T = len(sc.tri) // 2
    assert (cov.count == 2).all()
    assert (own["gbuffer"][0] >= T).all() and (own["rsm"][0] < T).all() and np.array_equal(own["gbuffer"][0] - T, own["rsm"][0])
    gb, _ = rt.oracle_gbuffer("same-depth", "z")
    assert np.array_equal(gb["depth"].view(np.uint32), ex.depth_bits(own["gbuffer"][1]))
    rt.assert_owner(gb["color"], sc, own["gbuffer"][0], "G-buffer colour, equal depths")
    rsm, _ = rt.oracle_rsm("same-depth", "z")
    assert np.array_equal(rsm["depth"][0], ex.d16_code(own["rsm"][1]))
    rt.assert_owner(rsm["flux"][0], sc, own["rsm"][0], "RSM flux, equal depths")


def _numpy_motion_reference():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gen_golden_motion_vectors as gmv
    return gmv


def test_motion_vectors_fp32_restatement_of_instanced_draws():
    """the same for draws through a model matrix with a whole-pixel translation (tests/test_raster_regrow_gpu.py): the vertex stage's one
    fp32 addition is part of the restatement"""
    gmv = _numpy_motion_reference()
    block, offsets = ex.instanced(100, 120, 7, (4, 8), "instanced-s7", mixed_winding=False)
    block = block.as_class(ex.SOLID)
    flat = ex.flatten(block, offsets)
    cov = ex.coverage(flat)
    owner, depth_n = ex.owners(flat, cov, "gbuffer")
    assert (cov.count == 1).all() and len(offsets) == 12
    depth = ex.depth_bits(depth_n).view(np.float32).copy()
    depth[::2, ::3] = 0.8751  # the depth of no fragment
    wins = np.ones(depth.shape, bool)
    wins[::2, ::3] = False
    want = rt.motion_vectors_fp32(flat, owner, wins, rt.MOTION_SHIFT, rt.instanced_world(block, offsets))
    got = gmv.motion_vectors(ex.to_mesh(block, offsets), rt.identity_view(100, 120, rt.MOTION_SHIFT), depth)
    assert np.array_equal(got, want) and np.array_equal((got != 0).any(-1), wins)


def test_motion_vectors_fp32_restatement_equals_the_numpy_reference():
    """the per-owner fp32 restatement the GPU tests compare the motion vectors with, against the project's numpy reference of that pass
    (tools/gen_golden_motion_vectors.py, one full-image evaluation per triangle: affordable for the sparsest case only)"""
    gmv = _numpy_motion_reference()
    name = "jitter-s40"
    sc, wins, want, depth_n = rt.motion_exact(name, "z")
    gb, _ = rt.oracle_gbuffer_of(rt.motion_mesh(name, "z").arrays(), sc.W, sc.H)
    assert np.array_equal(gb["depth"].view(np.uint32), ex.depth_bits(depth_n))
    st = {}
    got = gmv.motion_vectors(rt.motion_mesh(name, "z"), rt.identity_view(sc.W, sc.H, rt.MOTION_SHIFT), gb["depth"], st)
    assert np.array_equal(st["won"], wins) and 0.2 < wins.mean() < 0.8
    assert np.array_equal(got, want)
    assert (want[wins] != 0).any(-1).all()  # a whole-pixel shift: no vector of a kept pixel is zero
