"""sah_rt_refit (include/sah_rt_refit.h) on the device: the structure after a refit checked on its read-back (tests/rt_refit_check.py), and
rays through it against the brute-force oracle on the moved scene, bit for bit — the padded triangle box is part of the definition of a
hit, so a refit structure must answer exactly as a rebuilt one and as a test of every triangle."""
import ctypes as C

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, lib, mesh, synth
from tests import rt_structure_scenes as scenes
from tests.rt_refit_check import check_refit, moved
from tests.rt_structure_check import _bits
from tests.test_rt import RtCase, _probe_ids
from tests.support import side_stream_context

W, H, PROBES = 32, 18, 6


def _same_structure(a, b):
    return a["header"] == b["header"] and np.array_equal(_bits(a["nodes"]), _bits(b["nodes"])) and \
        np.array_equal(a["tris"].view(np.uint32), b["tris"].view(np.uint32))


def _case(m, surface=None, **kw):
    """an RtCase of `m`; surface: the case whose G-buffer the rays leave from (default: m's own, rasterised by the oracle)"""
    return RtCase(m, W, H, gbuffer=None if surface is None else {"depth": surface.gbuffer["depth"], "normals": surface.gbuffer["normals"]}, **kw)


def _hip_rays(ctx, case, probes):
    return [case.hip_rtao(ctx, 1, 4.0), case.hip_mask(ctx), case.hip_probe_trace(ctx, probes), *case.hip_rtgi(ctx)]


def _rays_equal_oracle(ctx, case, seed=9):
    """the four generators through the context's structure as it is (no build) == the oracle on the case's arrays"""
    probes = _probe_ids(seed, PROBES)
    got = _hip_rays(ctx, case, probes)
    want = [case.oracle_rtao(1, 4.0), case.oracle_mask(), case.oracle_probe_trace(probes), *case.oracle_rtgi()]
    for name, g, w in zip(("rtao", "shadow mask", "probe trace", "ray buffer", "ray irradiance"), got, want):
        assert g.tobytes() == w.tobytes(), f"{name} differs from the oracle"
    return got


def _refit_and_check(ctx, a_mesh, b_mesh, stats=False):
    """build over a_mesh, refit to b_mesh, check the structure -> (before, after, the device geometry of b_mesh)"""
    import torch
    keep = []
    ctx.rt_build(mesh.geometry(mesh.to_device(a_mesh.arrays()), keep))
    before = ctx.rt_structure()
    arrays = b_mesh.arrays()
    geo = mesh.geometry(mesh.to_device(arrays), keep)
    words = torch.full((4,), -1, dtype=torch.int32, device="cuda") if stats else None
    ctx.rt_refit(geo, words.data_ptr() if stats else None)
    after = ctx.rt_structure()
    present = check_refit(before, after, arrays, words.cpu().numpy().view(np.uint32).tolist() if stats else None)
    return before, after, present


@pytest.mark.gpu
@pytest.mark.parametrize("triangles", (1, 5, 257, 4097))
def test_identity(hip_ctx, triangles):
    """a refit to the arrays the structure was built over reproduces the build, triangles and nodes, bit for bit"""
    before, after, present = _refit_and_check(hip_ctx, scenes.soup(triangles), scenes.soup(triangles))
    assert present.all() and _same_structure(before, after)


# the issue's counts, and the kernel's own boundaries: one wave of the level kernel (64), its workgroup (256: a second launch above it)
BOUNDARY_COUNTS = (1, 4, 5, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097)


@pytest.mark.gpu
@pytest.mark.parametrize("triangles", BOUNDARY_COUNTS)
def test_triangle_count_boundaries(hip_ctx, triangles):
    a, b = _case(scenes.soup(triangles)), _case(moved(scenes.soup(triangles), seed=triangles))
    a.hip_build(hip_ctx)
    before = hip_ctx.rt_structure()
    hip_ctx.rt_refit(b.device()["geo"])
    after = hip_ctx.rt_structure()
    assert check_refit(before, after, b.arrays).all()
    assert after["pad_bits"] != before["pad_bits"] or triangles < 4
    _rays_equal_oracle(hip_ctx, b)


@pytest.mark.gpu
@pytest.mark.parametrize("triangles", (65536, 65537))
def test_more_levels_than_two_launches_cover(hip_ctx, triangles):
    """65 536 triangles: nine levels, the last two launches' worth; 65 537: ten levels, a third launch of the level kernel.  Structure only."""
    before, after, present = _refit_and_check(hip_ctx, scenes.soup(triangles), moved(scenes.soup(triangles)), stats=True)
    assert present.all() and before["num_levels"] == (9 if triangles == 65536 else 10)


def _remodelled(count):
    m = scenes.many_primitives(count)
    g = synth.rng(77)
    for p in m.primitives:
        p["model"] = scenes.rotation_y(float(g.uniform(0, 2 * np.pi)), g.uniform(-5, 5, 3))
    return m


@pytest.mark.gpu
def test_many_primitives(hip_ctx):
    """1025 primitives — instances, CUTOUT, bad index ranges, index counts that are no multiple of 3 — every model replaced"""
    import torch
    surface = RtCase(mesh.random_soup(31, triangles=400), W, H)
    a, b = _case(scenes.many_primitives(1025), surface, seed=9), _case(_remodelled(1025), surface, seed=9)
    for c in (a, b):
        c.sun.set_direction([0.3, -1.0, 0.2])
    a.hip_build(hip_ctx)
    before = hip_ctx.rt_structure()
    words = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    hip_ctx.rt_refit(b.device()["geo"], words.data_ptr())
    after = hip_ctx.rt_structure()
    stats = words.cpu().numpy().view(np.uint32).tolist()
    present = check_refit(before, after, b.arrays, stats)
    assert present.all() and stats[0] == before["num_tris"] and stats[1] == 0 and stats[3] == 0
    assert set(np.unique(after["tris"]["flags"])) == {0, 1}
    got = _rays_equal_oracle(hip_ctx, b)
    assert len(np.unique(got[0])) > 1 and len(np.unique(got[1])) > 1
    fresh = lib.Context(device=0)
    try:
        fresh.set_stream(torch.cuda.current_stream().cuda_stream)
        b.hip_build(fresh)
        rebuilt = _hip_rays(fresh, b, _probe_ids(9, PROBES))
        torch.cuda.synchronize()
    finally:
        fresh.close()
    for g, r in zip(got, rebuilt):
        assert g.tobytes() == r.tobytes(), "rays through the refit structure differ from rays through a fresh build"


@pytest.mark.gpu
def test_triangles_going_non_finite_and_coming_back(hip_ctx):
    import torch
    soup, broken = scenes.soup(2049, seed=14), scenes.non_finite()
    sa, ba = soup.arrays(), broken.arrays()
    assert np.array_equal(sa["indices"], ba["indices"]) and sa["primitives"].tobytes() == ba["primitives"].tobytes()
    same = sa["positions"].view(np.uint32) == ba["positions"].view(np.uint32)
    assert not np.isfinite(ba["positions"][~same]).any() and np.isfinite(ba["positions"][same]).all()  # same base positions
    a = _case(soup)
    b = _case(broken, a)
    a.hip_build(hip_ctx)
    before = hip_ctx.rt_structure()
    words = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    hip_ctx.rt_refit(b.device()["geo"], words.data_ptr())
    after = hip_ctx.rt_structure()
    stats = words.cpu().numpy().view(np.uint32).tolist()
    present = check_refit(before, after, b.arrays, stats)
    assert stats[0] + stats[1] == 2049 and 150 < stats[1] < 450 and int((~present).sum()) == stats[1]
    _rays_equal_oracle(hip_ctx, b)
    # and back: every triangle is present again
    hip_ctx.rt_refit(a.device()["geo"], words.data_ptr())
    back = hip_ctx.rt_structure()
    assert check_refit(after, back, a.arrays, words.cpu().numpy().view(np.uint32).tolist()).all()
    assert _same_structure(back, before)
    _rays_equal_oracle(hip_ctx, a)


@pytest.mark.gpu
def test_triangles_the_build_left_out_stay_out(hip_ctx):
    before, after, present = _refit_and_check(hip_ctx, scenes.non_finite(), scenes.soup(2049, seed=14), stats=True)
    assert present.all() and 2049 - 450 < after["num_tris"] == before["num_tris"] < 2049 - 150


@pytest.mark.gpu
def test_everything_absent(hip_ctx):
    """positions that are all NaN: every node absent, no ray hits anything (a defined input: the build accepts such scenes too)"""
    a = _case(scenes.soup(257))
    gone = scenes.soup(257)
    for pos in gone.positions:
        pos[...] = np.nan
    b = _case(gone, a)
    assert (a.gbuffer["depth"] > 0).mean() > 0.1
    a.hip_build(hip_ctx)
    before = hip_ctx.rt_structure()
    assert (a.hip_rtao(hip_ctx, 1, 4.0) == 0.0).any() and (a.hip_mask(hip_ctx) < 1.0).any()  # there is something to lose
    hip_ctx.rt_refit(b.device()["geo"])
    after = hip_ctx.rt_structure()
    assert not check_refit(before, after, b.arrays).any()
    assert (_bits(after["nodes"]) == 0x7f800000).all() and after["pad_bits"] == 0
    ao, mask = _rays_equal_oracle(hip_ctx, b)[:2]
    assert (ao == 1.0).all() and (mask == 1.0).all()
    hip_ctx.rt_refit(a.device()["geo"])
    assert _same_structure(hip_ctx.rt_structure(), before)


@pytest.mark.gpu
def test_pad_follows_the_scene(hip_ctx):
    """translated by (+1000, 0, 0) and back: the pad is this refit's both times, and the return gives the identity refit's nodes"""
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 1000.0
    before, identity, _ = _refit_and_check(hip_ctx, scenes.soup(1025), scenes.soup(1025))
    keep = []
    arrays = moved(scenes.soup(1025), displacement=0.0, model=far.T.reshape(16)).arrays()
    hip_ctx.rt_refit(mesh.geometry(mesh.to_device(arrays), keep))
    away = hip_ctx.rt_structure()
    check_refit(identity, away, arrays)
    pads = np.array([identity["pad_bits"], away["pad_bits"]], np.uint32).view(np.float32)
    assert pads[1] > 16 * pads[0]  # S went from < 16 to > 990
    arrays = scenes.soup(1025).arrays()
    hip_ctx.rt_refit(mesh.geometry(mesh.to_device(arrays), keep))
    back = hip_ctx.rt_structure()
    check_refit(away, back, arrays)
    assert _same_structure(back, identity)


def _copy_geo(geo, **fields):
    g = _abi.SceneGeometry()
    C.memmove(C.byref(g), C.byref(geo), C.sizeof(g))
    g._alive = geo._alive
    for k, v in fields.items():
        setattr(g, k, v)
    return g


@pytest.mark.gpu
def test_arguments(hip_ctx):
    import torch
    keep = []
    arrays = scenes.soup(17).arrays()
    geo = mesh.geometry(mesh.to_device(arrays), keep)
    fresh = lib.Context(device=0)
    try:
        with pytest.raises(lib.SahError) as e:  # no structure yet
            fresh.rt_refit(geo)
        assert e.value.status == _abi.SAH_ERR_INVALID_ARGUMENT and "sah_rt_build has not been called" in str(e.value)
    finally:
        fresh.close()
    hip_ctx.rt_build(geo)
    before = hip_ctx.rt_structure()
    for field in ("num_primitives", "num_vertices", "num_indices"):
        for delta in (1, -1):
            with pytest.raises(lib.SahError) as e:
                hip_ctx.rt_refit(_copy_geo(geo, **{field: getattr(geo, field) + delta}))
            assert e.value.status == _abi.SAH_ERR_INVALID_ARGUMENT
            assert _same_structure(hip_ctx.rt_structure(), before)
    # other addresses, the same contents
    hip_ctx.rt_refit(mesh.geometry(mesh.to_device(arrays), keep))
    assert _same_structure(hip_ctx.rt_structure(), before)
    # an empty scene: nothing to do
    empty = mesh.Mesh()
    empty.add_material(mesh.material())
    egeo = mesh.geometry(mesh.to_device(empty.arrays()), keep)
    assert hip_ctx.rt_build(egeo)[0] == 0
    words = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    hip_ctx.rt_refit(egeo)
    hip_ctx.rt_refit(egeo, words.data_ptr())
    assert words.cpu().tolist() == [0, 0, 0, 0] and hip_ctx.rt_structure()["num_tris"] == 0
    with pytest.raises(lib.SahError):
        hip_ctx.rt_refit(geo)  # 17 triangles against the empty structure's counts


@pytest.mark.gpu
def test_on_a_side_stream_without_host_sync_and_under_capture():
    """refit + RTAO recorded as one graph on a side stream; replayed twice with the positions overwritten in place in between: each
    replay's AO is the oracle's for the positions it found"""
    import torch
    a = _case(scenes.soup(1025))
    b1, b2 = _case(moved(scenes.soup(1025), seed=1), a), _case(moved(scenes.soup(1025), seed=2), a)
    want1, want2 = b1.oracle_rtao(1, 4.0), b2.oracle_rtao(1, 4.0)
    assert want1.tobytes() != want2.tobytes()
    with side_stream_context() as (ctx, s):
        dv = b1.device()  # b1's models and topology; its positions are what gets overwritten
        positions = dv["keep"][0]
        assert positions.numel() == b1.arrays["positions"].nbytes and positions.data_ptr() == dv["geo"].vertex_positions
        p1, p2 = (torch.from_numpy(np.frombuffer(c.arrays["positions"].tobytes(), np.uint8).copy()).cuda() for c in (b1, b2))
        out = torch.full((H, W), -7.0, dtype=torch.float32, device="cuda")
        d, n, z, o = b1.planes(dv["depth"], dv["normals"], dv["noise"], out)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.rt_build(a.device()["geo"])
            ctx.rt_refit(dv["geo"])
            ctx.rt_refit(dv["geo"])  # no host synchronisation in between
            ctx.rtao(b1.view.gpu_data, d, n, z, 1, 4.0, o)
        s.synchronize()
        assert out.cpu().numpy().tobytes() == want1.tobytes()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.rt_refit(dv["geo"])
            ctx.rtao(b1.view.gpu_data, d, n, z, 1, 4.0, o)
        for src, want in ((p2, want2), (p1, want1)):
            positions.copy_(src)
            out.fill_(-7.0)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == want.tobytes()
