"""The invariants A - E of tests/test_rt_structure_gpu.py on one read-back of the ray-tracing structure (Context.rt_structure()), and a
structure synthesised from the reference alone, with which tests/test_rt_structure_cpu.py checks the checker: it passes what is right and
names what is wrong."""
import numpy as np

from androidrenderer_amd import lib
from tests import rt_structure_ref as ref

INF_BITS = 0x7f800000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rows(tris):
    """TRIANGLE records as sorted rows of twelve words: a multiset that compares with array_equal"""
    w = np.ascontiguousarray(tris).view(np.uint32).reshape(-1, 12)
    return w[np.lexsort(w.T[::-1])]


def check_structure(stats, s, arrays):
    """A - E on one read-back; -> (kept, running, curve order) of the reference"""
    assert lib.RT_TRIANGLE == ref.TRIANGLE
    kept, running, dropped = ref.world_triangles(arrays)
    n = len(kept)
    tris, nodes = s["tris"], s["nodes"]
    # B
    offsets, counts = ref.level_table(n)
    assert stats[0] == s["num_tris"] == n == len(tris), (stats, s["num_tris"], n)
    assert stats[1] == dropped and stats[2] == s["num_levels"] == len(counts) and stats[3] == 0, (stats, dropped, len(counts))
    assert s["level_count"] == counts and s["level_offset"] == offsets
    assert s["header"][4 + len(counts):4 + lib.RT_MAX_LEVELS] == [0] * (lib.RT_MAX_LEVELS - len(counts))
    assert n == 0 or counts[-1] == 1
    assert nodes.shape[0] == (offsets[-1] + 1 if n else 0)
    assert s["pad_bits"] == ref.pad_bits(kept), (hex(s["pad_bits"]), hex(ref.pad_bits(kept)))
    # A
    assert np.array_equal(_rows(tris), _rows(kept)), "the structure's triangles are not the kept set"
    if n == 0:
        return kept, running, np.zeros(0, np.int64)
    # C
    pad = np.array(s["pad_bits"], np.uint32).view(np.float32)
    lo, hi = ref.boxes(tris)
    g0 = (n + 3) // 4
    lanes = nodes[:g0].transpose(0, 3, 1, 2).reshape(g0 * 4, 2, 3)  # (node, {lo, hi}, axis)
    assert np.array_equal(_bits(lanes[:n, 0]), _bits(lo - pad)) and np.array_equal(_bits(lanes[:n, 1]), _bits(hi + pad)), "level 0 boxes"
    assert (_bits(lanes[n:]) == INF_BITS).all(), "level 0: absent lanes"
    # D
    child = lanes[:n]
    for level in range(1, len(counts)):
        cnt, groups = counts[level], (counts[level] + 3) // 4
        full = np.empty((counts[level - 1] + 3) // 4 * 4, dtype=bool)
        full[:] = False
        full[:counts[level - 1]] = True
        padded = np.zeros((len(full), 2, 3), np.float32)
        padded[:counts[level - 1]] = child
        c = padded.reshape(-1, 4, 2, 3)
        exists = full.reshape(-1, 4)[:, :, None]
        want_lo = np.where(exists, c[:, :, 0], np.inf).min(axis=1).astype(np.float32)
        want_hi = np.where(exists, c[:, :, 1], -np.inf).max(axis=1).astype(np.float32)
        assert want_lo.shape[0] == cnt
        got = nodes[offsets[level]:offsets[level] + groups].transpose(0, 3, 1, 2).reshape(groups * 4, 2, 3)
        assert np.array_equal(_bits(got[:cnt, 0]), _bits(want_lo)) and np.array_equal(_bits(got[:cnt, 1]), _bits(want_hi)), f"level {level} boxes"
        assert (_bits(got[cnt:]) == INF_BITS).all(), f"level {level}: absent lanes"
        child = got[:cnt]
    # E
    base, _ = ref.tri_base(arrays["primitives"])
    at = base[tris["primitive"].astype(np.int64)] + tris["triangle"].astype(np.int64)  # running index of the triangle at each position
    order = ref.curve_order(kept, running)
    want = running[order]
    w = ref.REFINE_WINDOW
    for first in range(0, n, w):
        a, b = np.sort(at[first:first + w]), np.sort(want[first:first + w])
        assert np.array_equal(a, b), f"window {first // w}: {int(len(np.setdiff1d(a, b)))} triangles are not the key order's"
    return kept, running, order


def synthetic_structure(arrays, rng=None):
    """What a correct build would read back as, made from the reference: the key order, shuffled inside every refinement window when an
    rng is given (any such order is a correct build) -> (stats, structure)"""
    kept, running, dropped = ref.world_triangles(arrays)
    n = len(kept)
    order = ref.curve_order(kept, running)
    if rng is not None:
        for first in range(0, n, ref.REFINE_WINDOW):
            order[first:first + ref.REFINE_WINDOW] = rng.permutation(order[first:first + ref.REFINE_WINDOW])
    tris = kept[order]
    offsets, counts = ref.level_table(n)
    pad_bits = ref.pad_bits(kept)
    pad = np.array(pad_bits, np.uint32).view(np.float32)
    groups = offsets[-1] + 1 if n else 0
    nodes = np.full((groups * 4, 2, 3), np.inf, np.float32)  # (group lane, {lo, hi}, axis)
    lo, hi = ref.boxes(tris)
    lo, hi = lo - pad, hi + pad
    for level in range(len(counts)):
        nodes[4 * offsets[level]:4 * offsets[level] + counts[level], 0] = lo
        nodes[4 * offsets[level]:4 * offsets[level] + counts[level], 1] = hi
        parents = (counts[level] + 3) // 4
        plo, phi = np.full((parents * 4, 3), np.inf, np.float32), np.full((parents * 4, 3), -np.inf, np.float32)
        plo[:counts[level]], phi[:counts[level]] = lo, hi
        lo, hi = plo.reshape(parents, 4, 3).min(axis=1), phi.reshape(parents, 4, 3).max(axis=1)
    header = [n, len(counts), groups, pad_bits] + offsets + [0] * (lib.RT_MAX_LEVELS - len(counts)) + counts + [0] * (lib.RT_MAX_LEVELS - len(counts))
    s = {"num_tris": n, "num_levels": len(counts), "pad_bits": pad_bits, "level_offset": offsets, "level_count": counts, "header": header,
         "tris": tris, "nodes": np.ascontiguousarray(nodes.reshape(groups, 4, 2, 3).transpose(0, 2, 3, 1))}
    return [n, dropped, len(counts), 0], s
