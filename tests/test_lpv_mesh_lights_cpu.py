"""The LPV mesh lights (include/sah_lpv_mesh_lights.h) without a GPU: the library exports the three entries; the engine, the uniform and
the point cloud equal the numpy restatement (tools/gen_golden_mesh_lights.py) and libstdc++ itself; the entries answer made-up arguments
with a status code; the vectorised injection of the restatement is gen_golden.inject_vpls; the fixture regenerates bit for bit."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib, mesh, scene
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden as gg  # noqa: E402
import gen_golden_mesh_lights as gml  # noqa: E402

f32 = np.float32


def test_library_exports_the_mesh_light_entries_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.ML_EXPORTS)
    header = open(os.path.join(ROOT, "include", "sah_lpv_mesh_lights.h")).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.ML_EXPORTS)
    assert not set(lib.ML_EXPORTS) & set(lib.EXPORTS)
    assert f"(1u << 24)" in header and lib.LPV_EMISSIVE_MAX_ENTRIES == 1 << 24


def test_engine_known_answer():
    e = gml.MinStd0(1)
    for _ in range(9999):
        e()
    assert e() == 1043618065  # [rand.predef]: the 10000th consecutive invocation of a default-constructed minstd_rand0
    assert gml.MinStd0(0).x == 1 and gml.MinStd0(2147483647).x == 1 and gml.MinStd0(2147483648).x == 1


_DRAWS_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <random>
int main(int argc, char** argv) {
    std::default_random_engine e{std::strtoull(argv[1], nullptr, 10)};
    std::uniform_real_distribution<double> d{0.0, 1.0};
    for (int i = 0; i < 2000; i++) std::printf("%a\n", d(e));
}
"""


@pytest.mark.parametrize("seed", [0, 1, 1234, 2147483646, 2147483647, 2 ** 40 + 7, 2 ** 64 - 1])
def test_draws_equal_libstdcxx(tmp_path, seed):
    """the restatement's uniform over the engine is libstdc++'s uniform_real_distribution<double> over std::default_random_engine{seed};
    the library's points follow from the same draws (test_point_cloud_equals_restatement)"""
    src, exe = tmp_path / "draws.cpp", tmp_path / "draws"
    src.write_text(_DRAWS_CPP)
    cxx = next(c for c in ("g++", "c++", "/opt/rocm/llvm/bin/clang++") if subprocess.run(["which", c], capture_output=True).returncode == 0 or os.path.exists(c))
    subprocess.check_call([cxx, "-O2", "-std=c++17", str(src), "-o", str(exe)], timeout=300)
    want = [float.fromhex(x) for x in subprocess.check_output([str(exe), str(seed)], text=True).split()]
    e = gml.MinStd0(seed)
    got = [gml.uniform01(e) for _ in range(2000)]
    assert got == want


def _tri_mesh(tris):
    """host arrays of a triangle soup: tris (n, 3, 3)"""
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    pos = tris.reshape(-1, 3)
    vd = np.zeros(pos.shape[0], mesh.VERTEX_DATA)
    g = np.random.default_rng(len(pos))
    vd["normal"] = g.uniform(-1, 1, (len(pos), 3))
    vd["tangent"] = g.uniform(-1, 1, (len(pos), 4))
    vd["texcoord"] = g.uniform(-2, 2, (len(pos), 2))
    vd["color"] = g.integers(0, 2 ** 32, len(pos), dtype=np.uint64).astype(np.uint32)
    return pos, vd, np.arange(len(pos), dtype=np.uint32)


def _same(x, y):
    return [np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(x, y)]


def _check(pos, vd, idx, seed, flags, first=0, count=None, voff=0):
    count = len(idx) if count is None else count
    want = gml.point_cloud(pos, vd, idx, first, count, voff, seed, flags)
    got = lib.mesh_point_cloud(pos, vd, idx, first, count, voff, seed, flags)
    assert all(_same(want, got)), _same(want, got)
    return got


@pytest.mark.parametrize("flags", [0, lib.POINT_CLOUD_ON_SURFACE])
def test_point_cloud_equals_restatement(flags):
    # a single triangle, area 2: 20 points; default: between 1/3 and 0.58 of the way from the origin; on surface: on the triangle
    pos, vd, idx = _tri_mesh([[[1, 0, 0], [1, 2, 0], [1, 0, 2]]])
    p, pts, lo, hi = _check(pos, vd, idx, 5, flags)
    assert len(p) == 20 and list(lo) == [1, 0, 0] and list(hi) == [1, 2, 2]
    if flags:
        assert np.all(np.abs(p[:, 0] - 1) < 1e-6) and np.all(p[:, 1] + p[:, 2] <= 2 + 1e-5)
    else:
        assert np.all((p[:, 0] > 0.33) & (p[:, 0] < 0.58))
    # the atrium, every box, with a vertex offset into the shared streams
    a = mesh.atrium().arrays()
    for pr in a["primitives"][::5]:
        _check(a["positions"], a["vertex_data"], a["indices"], 77, flags, int(pr["first_index"]), int(pr["index_count"]), int(pr["vertex_offset"]))
    # a random soup with degenerate triangles between the others: those are never chosen
    g = np.random.default_rng(3)
    tris = g.uniform(-3, 3, (60, 3, 3)).astype(f32)
    tris[5::7, 1] = tris[5::7, 0]  # zero area
    pos, vd, idx = _tri_mesh(tris)
    p, pts, lo, hi = _check(pos, vd, idx, 99, flags)
    want = gml.point_cloud(pos, vd, idx, 0, len(idx), 0, 99, flags)
    assert len(p) > 1000


def test_degenerate_triangles_are_never_chosen():
    tris = np.zeros((5, 3, 3), f32)
    tris[1] = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
    tris[3] = [[0, 0, 1], [4, 0, 1], [0, 4, 1]]  # 0, 2 and 4 degenerate
    pos, vd, idx = _tri_mesh(tris)
    p, pts, _, _ = _check(pos, vd, idx, 11, lib.POINT_CLOUD_ON_SURFACE)
    z = p[:, 2]
    assert len(p) == 160 and np.all(np.isclose(z, 0, atol=1e-6) | np.isclose(z, 1, atol=1e-6))
    assert not np.any(np.all(p == 0, axis=1))  # a point of a degenerate (all-zero) triangle would be the origin


def test_sample_exactly_on_a_prefix_takes_the_next_triangle():
    """a sample lying exactly on a prefix goes to the NEXT triangle (the first prefix greater than the sample).  Seed 1745007098 makes the
    first draw u a dyadic rational of at most 24 significant bits (found by a search over the engine's states), so three triangles with
    float areas u * 4, then the rest of 4 in two parts, give prefix[0] == u exactly"""
    seed = 1745007098
    u = gml.uniform01(gml.MinStd0(seed))
    k, den = u.as_integer_ratio()
    assert k < 2 ** 24 and den & (den - 1) == 0
    rest = den - k
    hi_part = rest - rest % (1 << max(rest.bit_length() - 24, 0))
    areas = [k, hi_part, rest - hi_part]
    assert all(a < 2 ** 24 or a % (1 << (a.bit_length() - 24)) == 0 for a in areas)
    scale = 4.0 / den  # total area 4: 40 points
    tris = [[[0, 0, z], [2 * a * scale, 0, z], [0, 1, z]] for a, z in zip(areas, (0.0, 5.0, 9.0))]
    pos, vd, idx = _tri_mesh(tris)
    assert float(np.cumsum(np.array(areas, np.float64) * scale / 4.0)[0]) == u  # prefix[0] == u
    p, _, _, _ = _check(pos, vd, idx, seed, lib.POINT_CLOUD_ON_SURFACE)
    assert len(p) == 40 and p[0, 2] == 5.0  # triangle 1, not 0


def test_cap_and_empty_clouds():
    # 65,536 points at most: a 100 x 100 square has area 10,000, i.e. 100,000 at one point per 0.1
    pos, vd, idx = _tri_mesh([[[0, 0, 0], [100, 0, 0], [0, 100, 0]], [[100, 0, 0], [100, 100, 0], [0, 100, 0]]])
    p, _, _, _ = _check(pos, vd, idx, 3, 0)
    assert len(p) == 65536
    # zero and NaN area: no points
    pos, vd, idx = _tri_mesh([[[0, 0, 0], [1, 1, 1], [2, 2, 2]]])
    assert len(_check(pos, vd, idx, 3, 0)[0]) == 0
    pos, vd, idx = _tri_mesh([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]]])
    p, _, lo, hi = _check(pos, vd, idx, 3, 0)
    assert len(p) == 0 and list(lo) == [0, 0, 0] and list(hi) == [1, 1, 0]  # NaN coordinates do not enter the bounds
    # an empty range
    p, _, lo, hi = lib.mesh_point_cloud(pos, vd, idx, 0, 0, 0, 3)
    assert len(p) == 0 and np.all(lo == np.inf) and np.all(hi == -np.inf)


def test_point_cloud_refuses_bad_ranges_and_capacities():
    pos, vd, idx = _tri_mesh([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    L = lib.load()
    cnt = C.c_uint32(0)
    out_p, out_v = np.zeros((4, 3), f32), np.zeros(4, mesh.VERTEX_DATA)
    call = lambda *a: L.sah_mesh_point_cloud(pos.ctypes.data, vd.ctypes.data, 3, idx.ctypes.data, 3, *a, C.byref(cnt), None, None)
    assert call(0, 3, 0, 1, 0, out_p.ctypes.data, out_v.ctypes.data, 4) == _abi.SAH_ERR_INVALID_ARGUMENT and cnt.value == 5  # 5 points, room for 4
    assert call(0, 3, 1, 1, 0, None, None, 0) == _abi.SAH_ERR_INVALID_ARGUMENT  # vertex 3 is beyond the stream
    assert call(0, 2, 0, 1, 0, None, None, 0) == _abi.SAH_ERR_INVALID_ARGUMENT  # not a multiple of 3
    assert call(3, 3, 0, 1, 0, None, None, 0) == _abi.SAH_ERR_INVALID_ARGUMENT  # beyond the index array
    assert call(0, 3, 0, 1, 2, None, None, 0) == _abi.SAH_ERR_INVALID_ARGUMENT  # unknown flag
    assert call(0, 3, 0, 1, 0, out_p.ctypes.data, None, 4) == _abi.SAH_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("seed", [31, 32])
def test_no_argument_combination_crashes_a_mesh_light_entry(seed):
    support.run_fuzz_child("ml_fuzz_child.py", seed, 1500)


def _random_vpls(g, n, spread=20.0):
    pos = g.uniform(-spread, spread, (n, 3)).astype(np.float16).view(np.uint16).astype(np.uint32)
    col = g.uniform(0, 3, (n, 3)).astype(np.float16).view(np.uint16).astype(np.uint32)
    col[g.random(n) < 0.05] = 0
    nrm = g.integers(-127, 128, (n, 3)) & 0xFF
    nrm[g.random(n) < 0.05] = 0  # length(normalize(0)) is NaN: not < 1, kept
    out = np.zeros((n, 4), np.uint32)
    out[:, 0] = pos[:, 0] | (pos[:, 1] << 16)
    out[:, 1] = pos[:, 2] | (col[:, 0] << 16)
    out[:, 2] = col[:, 1] | (col[:, 2] << 16)
    out[:, 3] = nrm[:, 0] | (nrm[:, 1] << 8) | (nrm[:, 2] << 16)
    return out


def test_vectorised_injection_is_gen_golden_inject_vpls():
    view = scene.SceneView.default(640, 360)
    sun = scene.DirectionalLight()
    lpv = scene.LpvCascades()
    lpv.update_cascade_transforms(view, sun)
    g = np.random.default_rng(5)
    vpls = _random_vpls(g, 600, 6.0)
    vpls[300:400, :2] = vpls[300, :2]  # one cell takes 100 lights
    for c in (0, 1, 3):
        a = [g.uniform(-1, 1, (32, 32, 128, 4)).astype(np.float16) for _ in range(3)]
        b = [v.copy() for v in a]
        gg.inject_vpls(vpls, lpv.matrices[c], c, 4, a)
        gml.inject_vpls_fast(vpls, lpv.matrices[c], c, 4, b)
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint16), y.view(np.uint16))


def test_cascade_bounds_are_the_snapped_offset_plus_minus_half_the_size():
    view = scene.SceneView.default(640, 360)
    lpv = scene.LpvCascades()
    lpv.update_cascade_transforms(view, scene.DirectionalLight())
    for c in range(4):
        lo, hi = np.array(lpv.bounds[c].min_bounds[:]), np.array(lpv.bounds[c].max_bounds[:])
        assert np.allclose(hi - lo, 8.0 * 2 ** c)
        w2c = np.array(lpv.matrices[c].world_to_cascade[:], f32)
        assert np.allclose(gg.mat_vec(w2c, [f32(lo[0]), f32(lo[1]), f32(lo[2]), f32(1)])[:3], 0.25, atol=1e-6)  # the corners of the cascade
        assert np.allclose(gg.mat_vec(w2c, [f32(hi[0]), f32(hi[1]), f32(hi[2]), f32(1)])[:3], 0.75, atol=1e-6)


def test_fixture_regenerates_bit_identically():
    want = np.load(gml.FIXTURE)
    got = gml.atrium_fixture()
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert np.array_equal(want[k], got[k]), k
    assert np.count_nonzero(want["quirk_volumes"]) and not np.array_equal(want["quirk_volumes"], want["surface_volumes"])
