"""What sah_rt_refit (include/sah_rt_refit.h) must leave behind, checked on two read-backs of the structure (Context.rt_structure()): the
one before the refit and the one after it, against tests/rt_structure_ref.py on the scene arrays the refit was given.  Bit patterns
throughout.  synthetic_refit makes a correct "after" from the reference alone, with which tests/test_rt_refit_cpu.py checks this checker.

  1  the triangle count, the level tables and every position's (primitive, triangle, flags) are the build's
  2  a present position holds the reference's world triangle of its (primitive, triangle) in the new arrays; an absent one holds zeros
  3  pad = S * 2^-16 over the present triangles
  4  level 0: the triangle's box -+ pad, or the absent box [+inf, +inf]
  5  upper levels: min / max over the children that exist and are present; absent without one; lanes beyond a level's count absent"""
import numpy as np

from tests import rt_structure_ref as ref
from tests.rt_structure_check import INF_BITS, _bits

VERTS = ("v0", "v1", "v2")


def _lanes(nodes, offset, count):
    """(node, {lo, hi}, axis) of the ceil(count / 4) groups of one level, absent trailing lanes included"""
    groups = (count + 3) // 4
    return nodes[offset:offset + groups].transpose(0, 3, 1, 2).reshape(groups * 4, 2, 3)


def reference_triangles(tris, arrays):
    """the structure's positions against the new arrays -> (present mask, TRIANGLE records: the reference's world triangle where present,
    zero vertices elsewhere; ids and flags are the structure's)"""
    kept, running, _ = ref.world_triangles(arrays)
    base, _ = ref.tri_base(arrays["primitives"])
    p = tris["primitive"].astype(np.int64)
    inside = p < len(base)
    at = np.where(inside, base[np.where(inside, p, 0)] + tris["triangle"].astype(np.int64), -1)  # running index of each position
    where = np.searchsorted(running, at)
    where[where >= len(running)] = 0
    present = inside & (len(running) > 0)
    if len(running):
        present &= running[where] == at
        present &= (kept["primitive"][where] == tris["primitive"]) & (kept["triangle"][where] == tris["triangle"])
    want = np.zeros(len(tris), ref.TRIANGLE)
    want["primitive"], want["triangle"], want["flags"] = tris["primitive"], tris["triangle"], tris["flags"]
    for k in VERTS:
        if present.any():
            want[k][present] = kept[k][where[present]]
    return present, want


def refit_nodes(want, present, offsets, counts):
    """the node groups a refit leaves for these triangles -> (groups, {lo, hi}, axis, lane) float32"""
    n = len(want)
    pad = np.array(ref.pad_bits(want[present]), np.uint32).view(np.float32)
    groups = offsets[-1] + 1 if n else 0
    nodes = np.full((groups * 4, 2, 3), np.inf, np.float32)
    lo, hi = ref.boxes(want)
    lo, hi = np.where(present[:, None], lo - pad, np.inf).astype(np.float32), np.where(present[:, None], hi + pad, np.inf).astype(np.float32)
    here = present
    for level in range(len(counts)):
        nodes[4 * offsets[level]:4 * offsets[level] + counts[level], 0] = lo
        nodes[4 * offsets[level]:4 * offsets[level] + counts[level], 1] = hi
        parents = (counts[level] + 3) // 4
        plo, phi = np.full((parents * 4, 3), np.inf, np.float32), np.full((parents * 4, 3), -np.inf, np.float32)
        plo[:counts[level]] = np.where(here[:, None], lo, np.inf)
        phi[:counts[level]] = np.where(here[:, None], hi, -np.inf)
        any_child = np.zeros(parents * 4, bool)
        any_child[:counts[level]] = here
        here = any_child.reshape(parents, 4).any(axis=1)
        lo, hi = plo.reshape(parents, 4, 3).min(axis=1), phi.reshape(parents, 4, 3).max(axis=1)
        hi = np.where(here[:, None], hi, np.inf).astype(np.float32)
    return np.ascontiguousarray(nodes.reshape(groups, 4, 2, 3).transpose(0, 2, 3, 1))


def check_refit(before, after, arrays_after, stats=None):
    """1 - 5 on the read-backs before and after one refit to `arrays_after`; stats: the four words sah_rt_refit wrote, if it was asked to.
    -> the present mask per position"""
    # 1
    n = before["num_tris"]
    assert after["num_tris"] == n == len(after["tris"]), "triangle count changed"
    assert after["num_levels"] == before["num_levels"] and after["level_offset"] == before["level_offset"] and after["level_count"] == before["level_count"], \
        "level tables changed"
    assert after["header"][:3] == before["header"][:3] and after["header"][4:] == before["header"][4:], "header changed"
    offsets, counts = ref.level_table(n)
    assert after["level_offset"] == offsets and after["level_count"] == counts
    assert after["nodes"].shape == before["nodes"].shape == ((offsets[-1] + 1 if n else 0), 2, 3, 4)
    for k in ("primitive", "triangle", "flags"):
        assert np.array_equal(after["tris"][k], before["tris"][k]), f"ids: '{k}' changed at {int((after['tris'][k] != before['tris'][k]).sum())} positions"
    # 2
    present, want = reference_triangles(after["tris"], arrays_after)
    for k in VERTS:
        same = (_bits(after["tris"][k]) == _bits(want[k])).all(axis=1) if n else np.zeros(0, bool)
        assert same[present].all(), f"vertices: {int((~same[present]).sum())} present triangles are not the reference's ({k})"
        assert same[~present].all(), f"vertices: {int((~same[~present]).sum())} absent triangles do not hold zeros ({k})"
    # 3
    s = np.float32(0.0)
    if present.any():
        s = max(np.float32(np.abs(want[k][present]).max()) for k in VERTS)
    want_pad = ref.pad_bits(want[present])
    assert after["pad_bits"] == want_pad, f"pad: {after['pad_bits']:#x}, the present triangles give {want_pad:#x}"
    if stats is not None:
        assert list(stats) == [int(present.sum()), int((~present).sum()), int(np.array(s, np.float32).view(np.uint32)), 0], ("stats", list(stats))
    if n == 0:
        return present
    # 4, 5
    wn = refit_nodes(want, present, offsets, counts)
    for level in range(len(counts)):
        got, exp = _lanes(after["nodes"], offsets[level], counts[level]), _lanes(wn, offsets[level], counts[level])
        cnt = counts[level]
        wrong = (_bits(got[:cnt]) != _bits(exp[:cnt])).any(axis=(1, 2))
        assert not wrong.any(), f"level {level} boxes: {int(wrong.sum())} of {cnt} nodes differ, first {int(np.flatnonzero(wrong)[0])}"
        assert (_bits(got[cnt:]) == INF_BITS).all(), f"level {level}: absent lanes"
    return present


def synthetic_refit(before, arrays_after):
    """what a correct refit of `before` to `arrays_after` reads back as, from the reference alone"""
    present, want = reference_triangles(before["tris"], arrays_after)
    after = dict(before)
    after["tris"] = want
    after["pad_bits"] = ref.pad_bits(want[present])
    after["header"] = list(before["header"])
    after["header"][3] = after["pad_bits"]
    after["nodes"] = refit_nodes(want, present, before["level_offset"], before["level_count"])
    return after


def moved(m, seed=1, displacement=0.5, model=None):
    """`m` (a mesh.Mesh nobody else holds) with every vertex displaced by up to `displacement` per axis and every primitive under `model`
    (default: a rotation about y with a translation) — same topology, other coordinates.  -> m"""
    from androidrenderer_amd import synth
    from tests.rt_structure_scenes import rotation_y
    g = synth.rng(seed)
    for pos in m.positions:
        pos += g.uniform(-displacement, displacement, pos.shape).astype(np.float32)
    for p in m.primitives:
        p["model"] = rotation_y(0.7, (0.4, -0.3, 0.6)) if model is None else model
    return m
