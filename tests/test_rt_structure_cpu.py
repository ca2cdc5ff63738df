"""CPU: the checker of the ray-tracing build is itself checked — the numpy restatement (tests/rt_structure_ref.py) on hand-computed
examples, the properties of its Hilbert function, and against the oracle's kept / left-out counts; the invariants
(tests/rt_structure_check.py) on structures synthesised from the restatement, right ones and broken ones."""
import ctypes as C
import itertools

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib, mesh, synth
from tests import rt_structure_check as check
from tests import rt_structure_ref as ref
from tests import rt_structure_scenes as scenes
from tests import util


@pytest.mark.parametrize("bits", [3, 5])
def test_hilbert_index_is_a_bijection_whose_steps_are_face_neighbours(bits):
    side = 1 << bits
    cells = np.array(list(itertools.product(range(side), repeat=3)), np.uint32)
    index = ref.hilbert_index(cells, bits)
    assert len(cells) == side ** 3 and (side != 8 or len(cells) == 512)
    assert np.array_equal(np.sort(index), np.arange(side ** 3, dtype=np.uint64))  # distinct, and exactly 0 .. side^3 - 1
    along = cells[np.argsort(index)].astype(np.int64)
    assert (np.abs(np.diff(along, axis=0)).sum(axis=1) == 1).all()  # consecutive indices: one step along one axis
    assert tuple(along[0]) == (0, 0, 0)


def test_level_table_by_hand():
    assert ref.level_table(0) == ([], [])
    assert ref.level_table(1) == ([0], [1])
    assert ref.level_table(4) == ([0, 1], [4, 1])
    assert ref.level_table(5) == ([0, 2, 3], [5, 2, 1])
    assert ref.level_table(17) == ([0, 5, 7, 8], [17, 5, 2, 1])
    # 4097 triangles in 1025 groups, 1025 nodes in 257, 257 in 65, 65 in 17, 17 in 5, 5 in 2, 2 in 1, and the top node's own group
    assert ref.level_table(4097) == ([0, 1025, 1282, 1347, 1364, 1369, 1371, 1372], [4097, 1025, 257, 65, 17, 5, 2, 1])


def _flat(x0, x1, z=0.0, top=0.0):
    """a triangle whose box is [x0, x1] x [0, 1] x [z, top]"""
    return [(x0, 0.0, z), (x1, 0.0, z), (x0, 1.0, top)]


def _mesh_of(triangles, **kw):
    m = mesh.Mesh()
    mat = m.add_material(mesh.material())
    pos = np.array(triangles, np.float32).reshape(-1, 3)
    m.add_primitive(pos, [(0, 0, 1)] * len(pos), np.arange(len(pos)), mat, **kw)
    return m


def test_pad_by_hand():
    # the largest |coordinate| is 9 (negative): 9 * 2^-16 = 1.125 * 2^-13 -> exponent 127 - 13 = 0x72, mantissa 0.125 = 0x100000
    kept, running, dropped = ref.world_triangles(_mesh_of([_flat(0, 1), [(2.0, -9.0, 1.0), (3.0, 0.5, 8.5), (0.0, 0.0, 0.0)]]).arrays())
    assert len(kept) == 2 and dropped == 0 and ref.pad_bits(kept) == 0x39100000
    assert ref.pad_bits(kept[:0]) == 0


def test_tree_cost_by_hand():
    # four flat unit triangles side by side and a fifth far away with a height of 2.  Level 1: node 0 = [0, 4] x [0, 1] x [0, 0], half area
    # 4 * 1 = 4; node 1 = [10, 11] x [0, 1] x [0, 2]: 1 * 1 + 1 * 2 + 2 * 1 = 5.  Level 2, the root: [0, 11] x [0, 1] x [0, 2]: 11 + 2 + 22 = 35
    tris = [_flat(0, 1), _flat(1, 2), _flat(2, 3), _flat(3, 4), _flat(10, 11, 0.0, 2.0)]
    kept, _, _ = ref.world_triangles(_mesh_of(tris).arrays())
    assert ref.tree_cost(kept) == (4.0 + 5.0 + 35.0) / 35.0
    # the far one in the first group: node 0 = the root's box (35), node 1 = one flat triangle (1)
    assert ref.tree_cost(kept[[0, 1, 2, 4, 3]]) == (35.0 + 1.0 + 35.0) / 35.0
    assert ref.tree_cost(kept[:1]) == 0.0 and ref.tree_cost(kept[:4]) == 1.0  # one leaf: nothing above level 0; one group: the root alone


def test_world_triangles_by_hand():
    m = mesh.Mesh()
    mat = m.add_material(mesh.material())
    pos = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (float("nan"), 0, 0), (float("inf"), 1, 1)]
    model = np.eye(4, dtype=np.float32)
    model[:3, 3] = (10.0, 20.0, 30.0)
    model[0, 0] = 2.0
    # seven indices: two triangles and a stray index; the second triangle has the NaN vertex
    m.add_primitive(pos, [(0, 0, 1)] * 5, (0, 1, 2, 0, 1, 3, 4), mat, model=model.T.reshape(16), ptype=_abi.PRIMITIVE_TYPE_CUTOUT)
    m.add_primitive([(0, 0, 0)] * 3, [(0, 0, 1)] * 3, (0, 1), mat)                       # fewer than three indices: no triangle
    m.add_primitive([(5, 5, 5), (6, 5, 5), (5, 6, 5)], [(0, 0, 1)] * 3, (0, 1, 2, 0, 1, 9), mat)  # second triangle: vertex 9 is outside
    arrays = m.arrays()
    assert ref.tri_base(arrays["primitives"])[0].tolist() == [0, 2, 2] and ref.tri_base(arrays["primitives"])[1] == 4
    kept, running, dropped = ref.world_triangles(arrays)
    assert running.tolist() == [0, 2] and dropped == 2
    assert kept["primitive"].tolist() == [0, 2] and kept["triangle"].tolist() == [0, 0] and kept["flags"].tolist() == [1, 0]
    assert kept["v0"][0].tolist() == [10.0, 20.0, 30.0] and kept["v1"][0].tolist() == [12.0, 20.0, 30.0] and kept["v2"][0].tolist() == [10.0, 21.0, 30.0]
    assert kept["v2"][1].tolist() == [5.0, 6.0, 5.0]
    # an index range that runs past the end of the index array keeps the triangles that fit
    arrays["primitives"][2]["index_count"] = 300
    kept, running, dropped = ref.world_triangles(arrays)
    assert running.tolist() == [0, 2] and dropped == 1 + 99


def test_sort_key_by_hand():
    # centres on x at 0, 1, 2.5 and 10 (boxes [c - 0.5, c + 0.5]): q = trunc((c - 0) / 10 * 1023) = 0, 102, 255, 1023; no extent on y and z
    tris = [_flat(c - 0.5, c + 0.5) for c in (10.0, 0.0, 2.5, 1.0)]
    kept, running, _ = ref.world_triangles(_mesh_of(tris).arrays())
    q = ref.quantised_centres(kept)
    assert q[:, 0].tolist() == [1023, 0, 255, 102] and (q[:, 1:] == 0).all()
    # along one axis from the origin the curve's order is the coordinate's
    assert ref.curve_order(kept, running).tolist() == [1, 3, 2, 0]
    # equal keys: ties go by running index, whatever the order of the records
    same = np.concatenate([kept[:1]] * 5)
    assert ref.curve_order(same, np.array([7, 3, 9, 1, 5])).tolist() == [3, 1, 4, 0, 2]
    assert ref._unordered(ref._ordered(np.array([-0.0, 0.0, -1.5, 3.0, -np.inf], np.float32))).view(np.uint32).tolist() == \
        np.array([-0.0, 0.0, -1.5, 3.0, -np.inf], np.float32).view(np.uint32).tolist()
    assert np.argsort(ref._ordered(np.array([0.0, -0.0, 2.0, -3.0], np.float32))).tolist() == [3, 1, 0, 2]


@pytest.mark.parametrize("scene", ["many_primitives", "non_finite"])
def test_kept_set_agrees_with_the_oracle(scene):
    """an independent statement of the same rules (oracle/rt.cpp, a loop over primitives): counts and pad"""
    m = scenes.many_primitives(1025) if scene == "many_primitives" else scenes.non_finite()
    arrays = m.arrays()
    kept, running, dropped = ref.world_triangles(arrays)
    g = mesh.geometry(mesh.with_counts(arrays), [])
    stats, pad = (C.c_uint32 * 4)(), C.c_float()
    assert util.oracle().orc_rt_stats(C.byref(g), stats, C.byref(pad)) == 0
    assert [stats[0], stats[1]] == [len(kept), dropped] and dropped > 0
    assert int(np.array(pad.value, np.float32).view(np.uint32)) == ref.pad_bits(kept)


def _synthetic(m, shuffle=True):
    arrays = m.arrays()
    stats, s = check.synthetic_structure(arrays, synth.rng(3) if shuffle else None)
    return stats, s, arrays


@pytest.mark.parametrize("scene", ["soup_1", "soup_5", "soup_2049", "many_primitives", "duplicates", "non_finite"])
def test_checker_passes_a_correct_structure(scene):
    m = {"soup_1": lambda: scenes.soup(1), "soup_5": lambda: scenes.soup(5), "soup_2049": lambda: scenes.soup(2049),
         "many_primitives": lambda: scenes.many_primitives(1023), "duplicates": scenes.duplicates, "non_finite": scenes.non_finite}[scene]()
    check.check_structure(*_synthetic(m))


def test_checker_names_what_is_wrong():
    def broken(change, message):
        stats, s, arrays = _synthetic(scenes.soup(2049))
        change(stats, s)
        with pytest.raises(AssertionError, match=message):
            check.check_structure(stats, s, arrays)

    def lose_one(stats, s):  # what a wrong permutation in a refinement window does: one triangle twice, another gone
        s["tris"][1500] = s["tris"][1501]
    broken(lose_one, "not the kept set")

    def shrink_leaf(stats, s):
        s["nodes"][10, 1, 2, 3] = np.nextafter(s["nodes"][10, 1, 2, 3], np.float32(-np.inf))
    broken(shrink_leaf, "level 0 boxes")

    def shrink_upper(stats, s):
        s["nodes"][s["level_offset"][3], 0, 0, 0] = np.nextafter(s["nodes"][s["level_offset"][3], 0, 0, 0], np.float32(np.inf))
    broken(shrink_upper, "level 3 boxes")

    def absent(stats, s):  # 2049 triangles: lanes 1 .. 3 of level 0's last group stand for nothing
        s["nodes"][s["level_offset"][1] - 1, 1, 0, 2] = 0.0
    broken(absent, "level 0: absent lanes")

    def across_windows(stats, s):  # a correct hierarchy over an order the keys do not give
        s2 = dict(s)
        order = np.arange(2049)
        order[[5, 1030]] = order[[1030, 5]]
        tris = s["tris"][order]
        lo, hi = ref.boxes(tris)
        pad = np.array(s["pad_bits"], np.uint32).view(np.float32)
        nodes = s["nodes"].transpose(0, 3, 1, 2).reshape(-1, 2, 3).copy()
        lo, hi = lo - pad, hi + pad
        for level, (off, cnt) in enumerate(zip(s["level_offset"], s["level_count"])):
            nodes[4 * off:4 * off + cnt, 0], nodes[4 * off:4 * off + cnt, 1] = lo, hi
            n = (cnt + 3) // 4
            plo, phi = np.full((4 * n, 3), np.inf, np.float32), np.full((4 * n, 3), -np.inf, np.float32)
            plo[:cnt], phi[:cnt] = lo, hi
            lo, hi = plo.reshape(n, 4, 3).min(axis=1), phi.reshape(n, 4, 3).max(axis=1)
        s["tris"], s["nodes"] = tris, np.ascontiguousarray(nodes.reshape(-1, 4, 2, 3).transpose(0, 2, 3, 1))
    broken(across_windows, "window 0: 1 triangles")

    def miscount(stats, s):
        stats[1] += 1
    broken(miscount, None)


def test_read_back_needs_a_structure():
    """sah_debug_rt_structure on a context without a build fails the way the ray generators do (here: a context without a device)"""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        return  # a HIP device is present: tests/test_rt_structure_gpu.py::test_read_back_entry covers it there
    header = (C.c_uint32 * lib.RT_STRUCTURE_HEADER_WORDS)(*([7] * lib.RT_STRUCTURE_HEADER_WORDS))
    buf = np.full(64, 0xa5, np.uint8)
    inv = _abi.SAH_ERR_INVALID_ARGUMENT
    assert L.sah_debug_rt_structure(None, header, None, 0, None, 0) == inv
    assert L.sah_debug_rt_structure(h, header, None, 0, None, 0) == inv
    assert L.sah_debug_rt_structure(h, header, buf.ctypes.data, buf.nbytes, buf.ctypes.data, buf.nbytes) == inv
    assert b"sah_rt_build has not been called" in L.sah_last_error(h)
    view = _abi.ViewData()
    assert L.sah_rtao(h, C.byref(view), None, None, None, 1, 1.0, None) == inv and b"sah_rt_build has not been called" in L.sah_last_error(h)
    assert list(header) == [7] * lib.RT_STRUCTURE_HEADER_WORDS and (buf == 0xa5).all()
    L.sah_destroy(h)
