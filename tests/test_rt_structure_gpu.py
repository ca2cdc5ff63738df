"""The ray-tracing BUILD, checked on the structure itself (sah_debug_rt_structure) and not through rays: rays see the same results through
any hierarchy of enclosing boxes (include/sah_hip.h), so a lost triangle, a box too small, a sort that does not sort or a refinement that
makes the tree worse can all hide from tests/test_rt.py.  Every comparison is on bit patterns against tests/rt_structure_ref.py.

  A  the structure's triangles are a permutation of the reference's kept set        E  every aligned window of 1024 positions holds the set
  B  stats, triangle and level counts, the level table, one node on top                the reference's key order puts there (keys, both sorts;
  C  level 0: lane i % 4 of group i / 4 is triangle i's fp32 box -+ pad                the refinement permutes inside its window only)
  D  upper levels: exact min / max of the existing children; absent lanes +inf      F  the refinement lowers the tree cost
                                                                                    G  ray results on a long primitive list == the oracle"""
import ctypes as C

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib, mesh
from tests import rt_structure_ref as ref
from tests.rt_structure_check import check_structure, _bits, _rows
from tests import rt_structure_scenes as scenes
from tests.test_rt import RtCase, _check_both, _check_gi, _probe_ids


def build_and_read(ctx, m):
    """sah_rt_build over the mesh's arrays on the device, then the read-back; -> (stats, structure, host arrays)"""
    arrays = m.arrays()
    keep = []
    geo = mesh.geometry(mesh.to_device(arrays), keep)
    stats = ctx.rt_build(geo)
    return stats, ctx.rt_structure(), arrays


@pytest.mark.gpu
@pytest.mark.parametrize("triangles", scenes.BOUNDARY_COUNTS)
def test_triangle_count_boundaries(hip_ctx, triangles):
    stats, s, arrays = build_and_read(hip_ctx, scenes.soup(triangles))
    check_structure(stats, s, arrays)
    assert stats[0] == triangles and stats[1] == 0


@pytest.fixture(scope="module")
def long_list():
    """the 3000-primitive scene (shared by the structure, the cost and the ray tests; nothing changes it)"""
    return scenes.many_primitives(3000)


@pytest.mark.gpu
@pytest.mark.parametrize("primitives", scenes.PRIMITIVE_COUNTS)
def test_many_primitives(hip_ctx, primitives, long_list):
    m = long_list if primitives == 3000 else scenes.many_primitives(primitives)
    stats, s, arrays = build_and_read(hip_ctx, m)
    kept, running, _ = check_structure(stats, s, arrays)
    counts = arrays["primitives"]["index_count"]
    assert len(counts) == primitives and (counts % 3 != 0).any() and (counts < 3).any() and stats[1] >= 4 and stats[0] > primitives
    assert set(np.unique(kept["flags"])) == {0, 1}
    assert len(np.unique(kept["primitive"])) > primitives // 2


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["coincident_centres", "planar", "duplicates"])
def test_degenerate_extents(hip_ctx, kind):
    stats, s, arrays = build_and_read(hip_ctx, getattr(scenes, kind)())
    kept, running, order = check_structure(stats, s, arrays)
    q = ref.quantised_centres(kept)
    if kind == "planar":
        assert (q[:, 2] == 0).all() and q[:, 0].max() == 1023 and q[:, 1].max() == 1023
    else:
        assert (q == 0).all() and np.array_equal(order, np.arange(len(kept)))  # every key ties: the order is the running index
    if kind == "duplicates":
        assert stats[0] == 64 and len(np.unique(_rows(s["tris"])[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], axis=0)) == 1


@pytest.mark.gpu
def test_non_finite_vertices(hip_ctx):
    m = scenes.non_finite()
    stats, s, arrays = build_and_read(hip_ctx, m)
    kept, _, _ = check_structure(stats, s, arrays)
    assert stats[0] + stats[1] == 2049 and 150 < stats[1] < 450  # about 1 - 0.95^3 of the triangles
    assert np.isfinite(s["tris"]["v0"]).all() and np.isfinite(s["tris"]["v1"]).all() and np.isfinite(s["tris"]["v2"]).all()


@pytest.mark.gpu
def test_rebuild_on_one_context(hip_ctx):
    """the context's buffers are reused (and here mostly larger than the scene): nothing of an earlier build survives in a later one"""
    for triangles in (4097, 5, 2049):
        stats, s, arrays = build_and_read(hip_ctx, scenes.soup(triangles, seed=triangles))
        check_structure(stats, s, arrays)
        assert stats[0] == triangles


@pytest.mark.gpu
def test_read_back_entry(hip_ctx):
    """sah_debug_rt_structure: sizes from a call without buffers, a short buffer refused untouched, no structure -> the generators' error,
    and a read-back changes nothing (the next one is the same, the cache epoch stands)"""
    L = hip_ctx.lib
    fresh = lib.Context(device=0)
    with pytest.raises(lib.SahError) as e:
        fresh.rt_structure()
    assert e.value.status == _abi.SAH_ERR_INVALID_ARGUMENT
    fresh.close()
    stats, s, _ = build_and_read(hip_ctx, scenes.soup(17))
    epoch = hip_ctx.cache_epoch()
    header = (C.c_uint32 * lib.RT_STRUCTURE_HEADER_WORDS)()
    assert L.sah_debug_rt_structure(hip_ctx.handle, header, None, 0, None, 0) == 0
    assert list(header)[:3] == [17, 4, 5 + 2 + 1 + 1] and list(header) == s["header"]
    tris, nodes = np.full(17 * 12, 0xa5a5a5a5, np.uint32), np.full(9 * 24, 0x5a5a5a5a, np.uint32)
    sentinel = (C.c_uint32 * lib.RT_STRUCTURE_HEADER_WORDS)(*([7] * lib.RT_STRUCTURE_HEADER_WORDS))
    for tb, nb in ((tris.nbytes - 1, nodes.nbytes), (tris.nbytes, nodes.nbytes - 1), (0, 0)):
        assert L.sah_debug_rt_structure(hip_ctx.handle, sentinel, tris.ctypes.data, tb, nodes.ctypes.data, nb) == _abi.SAH_ERR_INVALID_ARGUMENT
        assert (tris == 0xa5a5a5a5).all() and (nodes == 0x5a5a5a5a).all() and list(sentinel) == [7] * lib.RT_STRUCTURE_HEADER_WORDS
    assert L.sah_debug_rt_structure(hip_ctx.handle, None, tris.ctypes.data, tris.nbytes, None, 0) == 0  # one array alone
    assert np.array_equal(tris, s["tris"].view(np.uint32)) and (nodes == 0x5a5a5a5a).all()
    again = hip_ctx.rt_structure()
    assert again["header"] == s["header"] and np.array_equal(_bits(again["nodes"]), _bits(s["nodes"])) and np.array_equal(_rows(again["tris"]), _rows(s["tris"]))
    assert hip_ctx.cache_epoch() == epoch


def _costs(ctx, m):
    stats, s, arrays = build_and_read(ctx, m)
    kept, running, order = check_structure(stats, s, arrays)
    return ref.tree_cost(s["tris"]), ref.tree_cost(kept[order])


@pytest.mark.gpu
def test_refinement_lowers_the_tree_cost_atrium(hip_ctx):
    """F.  mesh.atrium(8), 23 808 triangles: sum of node areas / root area of the built order against the key order alone.  No margin:
    lowering this figure is all the refinement is for; the test prints both figures.  The key order's cost is 30.7181 by the restatement
    alone (rt.hip quotes 31.3 -> 26.6 for this scene, from an experiment that quantised against the scene's box); the built order's figure
    is not measured yet: no MI355X run of this test has been possible."""
    built, curve = _costs(hip_ctx, mesh.atrium(8))
    print(f"atrium(8) tree cost: curve order {curve:.4f}, built {built:.4f}")
    assert built < curve, (built, curve)


@pytest.mark.gpu
def test_refinement_lowers_the_tree_cost_long_list(hip_ctx, long_list):
    """F on the 3000-primitive scene (4439 triangles); the test prints both figures.  The key order's cost is 52.4318 by the restatement
    alone; the built order's figure is not measured yet: no MI355X run of this test has been possible."""
    built, curve = _costs(hip_ctx, long_list)
    print(f"3000 primitives tree cost: curve order {curve:.4f}, built {built:.4f}")
    assert built < curve, (built, curve)


@pytest.mark.gpu
def test_rays_on_a_long_primitive_list(hip_ctx, long_list):
    """G.  Occlusion and GI rays through the structure of 3000 primitives == the oracle, bit for bit.  The G-buffer the rays leave from is
    a soup's (the oracle's rasteriser does not draw index counts that are no multiple of 3); the GI hit stage reads the material through
    the hit's primitive id, so a wrong find_primitive shows in the irradiance where occlusion would not notice."""
    surface = RtCase(mesh.random_soup(31, triangles=400), 32, 18)
    case = RtCase(long_list, 32, 18, seed=9, gbuffer={"depth": surface.gbuffer["depth"], "normals": surface.gbuffer["normals"]})
    case.sun.set_direction([0.3, -1.0, 0.2])
    assert (case.gbuffer["depth"] > 0).mean() > 0.3
    ao, mask = _check_both(hip_ctx, case, spp=1, radius=4.0)
    assert len(np.unique(ao)) > 1 and len(np.unique(mask)) > 1
    _, rb_o, ri_o = _check_gi(hip_ctx, case, _probe_ids(9, 6))
    traced = case.gbuffer["depth"] > 0
    assert len(np.unique(rb_o.view(np.uint16)[traced][:, 3])) > 2 and len(np.unique(ri_o.view(np.uint16)[traced][:, 0])) > 2
