"""LPV mesh lights on the GPU (include/sah_lpv_mesh_lights.h), bit for bit against the numpy restatement tools/gen_golden_mesh_lights.py:
the VPLs of emissive clouds (constant texels, SRGB / UNORM emission textures with mips and a sampler bias, both material modes, inf / NaN
emission); the injection of the atrium (against the committed fixture too) and of random soups under rotated and mirrored models with CUTOUT,
non-emissive and far-away primitives; the injection against per-cascade sah_lpv_inject_vpls calls on concatenated lists; a call of more
than a million entries with one cell taking over 100,000 adds; order onto filled volumes, repeatability and stream capture; and an atrium
LPV frame with mesh lights through propagation and the Lighting pass."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, lib, mesh, scene
from tests import util
from tests.support import side_stream_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_mesh_lights as gml  # noqa: E402

RGBA16 = _abi.FORMAT_R16G16B16A16_SFLOAT
SHAPE = (32, 32, 128, 4)


def _vol(t):
    return images.volume(t, RGBA16)


def _same(x, y):  # bit for bit, a NaN is a NaN whatever its payload
    x, y = np.asarray(x).view(np.uint16), np.asarray(y).view(np.uint16)
    xn, yn = (x & 0x7FFF) > 0x7C00, (y & 0x7FFF) > 0x7C00
    return bool(np.all((x == y) | (xn & yn)))


def _vpls_same(got, want):
    """PackedVPL words, NaN halves compared as NaN"""
    g16, w16 = np.asarray(got, np.uint32).view(np.uint16), np.asarray(want, np.uint32).view(np.uint16)
    return _same(g16, w16)


def _lpv(w=192, h=108):
    view = scene.SceneView.default(w, h)
    sun = scene.DirectionalLight(shadow_mode=_abi.SHADOW_MODE_CSM)
    lpv = scene.LpvCascades()
    lpv.update_cascade_transforms(view, sun)
    return view, sun, lpv


def _device_scene(arrays):
    dev = mesh.to_device(arrays)
    keep = []
    return mesh.geometry(dev, keep), keep


def _clouds(hip_ctx, arrays, seed, flags=0, vpl_flags=0):
    import torch
    g, keep = _device_scene(arrays)
    records, ck = mesh.emissive_clouds(hip_ctx, arrays, g, seed, flags, vpl_flags)
    torch.cuda.synchronize()
    host = [(util.from_torch(k["vpls"], np.uint32).reshape(-1, 4)[:r.count], r.primitive, k["bounds"][0], k["bounds"][1]) for r, k in zip(records, ck)]
    return g, records, host, (keep, ck)


def _inject(hip_ctx, g, records, lpv, prior=None, nc=4):
    import torch
    vols = prior if prior is not None else [np.zeros(SHAPE, np.uint16) for _ in range(3)]
    t = [util.to_torch(v.copy()) for v in vols]
    hip_ctx.lpv_inject_emissive(g, records, lpv.matrices, lpv.bounds, nc, [_vol(x) for x in t])
    torch.cuda.synchronize()
    return [util.from_torch(x, np.uint16).reshape(SHAPE) for x in t]


def _want(arrays, host, lpv, prior=None, nc=4):
    vols = [(v.copy() if prior is not None else np.zeros(SHAPE, np.uint16)).view(np.float16) for v in (prior or [None] * 3)]
    gml.inject_emissive(arrays, host, lpv.matrices, gml.cascade_bounds(lpv), nc, vols)
    return [v.view(np.uint16) for v in vols]


# ---- the VPL build -----------------------------------------------------------------------------------------------------------------
def _emissive_mesh(textured):
    g = np.random.default_rng(40)
    m = mesh.Mesh()
    tex = []
    if textured:
        tex.append(m.add_texture(*mesh.random_texture(g, 32, 16, None, True, mesh.sampler(bias=0.7))))                       # SRGB, trilinear
        tex.append(m.add_texture(*mesh.random_texture(g, 17, 9, 3, False, mesh.sampler(mag=0, min=0, mipmap=0, bias=-0.4, min_lod=0.5))))
        tex.append(m.add_texture(*mesh.random_texture(g, 64, 64, None, False, mesh.sampler(mag=1, min=1, mipmap=1, bias=1.6, max_lod=2.5,
                                                                                            address_u=_abi.ADDRESS_MIRRORED_REPEAT))))
    em = [(1.5, 0.5, 2.0, 1.0), (0.0, 3.0, 0.25, 0.0), (np.inf, 1.0, 0.0, 0.0), (np.nan, 2.0, 1.0, 0.0), (1.0e5, 1.0, 1.0, 0.0)]
    mats = []
    for i, e in enumerate(em):
        slot = tex[i % len(tex)] if textured else _abi.TEXTURE_NONE
        mat = mesh.material(emission=e)
        mat["emission_texel"] = (0.3 + 0.1 * i, 0.9, 0.5, 1.0)
        mats.append(m.add_material(mat, emission=slot))
    for i in range(6):
        pos = g.uniform(-2, 2, (30, 3)).astype(np.float32)
        rot = np.eye(4, dtype=np.float32)
        a = 0.7 * i
        rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
        rot[:3, 3] = g.uniform(-3, 3, 3)
        m.add_primitive(pos, g.normal(size=(30, 3)), np.arange(30), mats[i % len(mats)], model=rot.T.reshape(16),
                        texcoords=g.uniform(-2, 3, (30, 2)), colors=g.integers(0, 2 ** 32, 30, dtype=np.uint64).astype(np.uint32))
    return m.arrays()


@pytest.mark.parametrize("textured", [False, True])
@pytest.mark.parametrize("vpl_flags", [0, lib.EMISSIVE_MATERIAL_ZERO])
def test_emissive_vpls_equal_numpy(hip_ctx, textured, vpl_flags):
    """every primitive's VPLs, emissive or not (a NaN emission factor is not 'emissive' for the selection, but its VPLs are defined)"""
    import torch
    arrays = _emissive_mesh(textured)
    g, keep = _device_scene(arrays)
    cols = []
    for prim, p in enumerate(arrays["primitives"]):
        pos, pts, _, _ = lib.mesh_point_cloud(arrays["positions"], arrays["vertex_data"], arrays["indices"], int(p["first_index"]), int(p["index_count"]),
                                              int(p["vertex_offset"]), 9 + prim)
        assert len(pos) > 0
        pos_t, pts_t = util.to_torch(pos), util.to_torch(pts.view(np.uint8).reshape(-1))
        out = torch.zeros((len(pos), 4), dtype=torch.int32, device="cuda")
        hip_ctx.lpv_emissive_vpls(g, prim, pos_t.data_ptr(), pts_t.data_ptr(), len(pos), vpl_flags, out.data_ptr())
        torch.cuda.synchronize()
        got = util.from_torch(out, np.uint32).reshape(-1, 4)
        want = gml.emissive_vpls(arrays, prim, pos, pts, vpl_flags)
        assert _vpls_same(got, want), f"primitive {prim}"
        cols.append(_half(got[:, 1] >> 16))
    if not vpl_flags:  # inf and NaN emission reach the VPL colour as half inf / NaN (1e5 times a texel overflows half)
        assert np.isinf(cols[2]).any() and np.isnan(cols[3]).any() and np.isinf(cols[4]).any()


def _half(bits):
    return (np.asarray(bits, np.uint32) & 0xFFFF).astype(np.uint16).view(np.float16)


# ---- the injection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, lib.POINT_CLOUD_ON_SURFACE])
def test_atrium_injection_equals_numpy_and_fixture(hip_ctx, flags):
    arrays = mesh.atrium().arrays()
    view, sun, lpv = _lpv(1920, 1080)
    g, records, host, keep = _clouds(hip_ctx, arrays, 1234, flags)
    assert sum(r.count for r in records) * 4 <= 4096  # the single-workgroup form
    got = _inject(hip_ctx, g, records, lpv)
    want = _want(arrays, host, lpv)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), f"colour {c}: {int((got[c] != want[c]).sum())} halves differ"
    assert any(np.count_nonzero(v) for v in got)
    # the committed fixture (same camera, seed and flags) — computed by the restatement alone
    fx = np.load(gml.FIXTURE)
    tag = "surface" if flags else "quirk"
    assert np.array_equal(np.concatenate([h[0] for h in host]), fx[f"{tag}_vpls"])
    assert np.array_equal(np.stack(got), fx[f"{tag}_volumes"])


def _soup(triangles=240, size=(0.05, 1.5)):
    m = mesh.random_soup(71, triangles=triangles, extent=5.0, size=size, cutout_fraction=0.0)
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0]).astype(np.float32)
    mirror[:3, 3] = (0.5, 0.2, -0.3)
    m.add_instance(0, mirror.T.reshape(16))                      # mirrored: the two corners give min.x > max.x
    rot = np.eye(4, dtype=np.float32)
    rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1] = 0.0, -1.0, 1.0, 0.0
    m.add_instance(1, rot.T.reshape(16))                         # rotated by 90 degrees
    far = np.eye(4, dtype=np.float32)
    far[:3, 3] = (500.0, 0.0, 0.0)
    m.add_instance(2, far.T.reshape(16))                         # outside every cascade
    dark = m.add_material(mesh.material(emission=(0, 0, 0, 0)))
    m.add_instance(1, np.eye(4, dtype=np.float32).reshape(16), dark)  # not emissive
    cut = np.eye(4, dtype=np.float32)
    cut[:3, 3] = (0.0, 1.0, 0.0)
    m.add_instance(0, cut.T.reshape(16))
    m.primitives[-1]["type"] = _abi.PRIMITIVE_TYPE_CUTOUT       # emissive but CUTOUT: never selected
    return m.arrays()


def test_soup_injection_equals_numpy(hip_ctx):
    arrays = _soup()
    view, sun, lpv = _lpv()
    g, records, host, keep = _clouds(hip_ctx, arrays, 5, 0)
    prims = [r.primitive for r in records]
    assert prims == sorted(prims) and len(records) >= 9
    assert sum(r.count for r in records) * 4 > 4096  # the multi-workgroup form
    sel = [[gml.selected(arrays, (p, lo, hi), gml.cascade_bounds(lpv)[c]) for (_, p, lo, hi) in host] for c in range(4)]
    types = arrays["primitives"]["type"]
    assert not any(sel[c][i] for c in range(4) for i, p in enumerate(prims) if types[p] != _abi.PRIMITIVE_TYPE_SOLID)
    assert any(sel[0]) and not all(sel[0]) and any(not any(sel[c][i] for c in range(4)) for i in range(len(prims)))
    lo_hi = [gml.gg.mat_vec(arrays["primitives"][p]["model"].astype(np.float32), [np.float32(lo[0]), 0, 0, np.float32(1)])[0] >
             gml.gg.mat_vec(arrays["primitives"][p]["model"].astype(np.float32), [np.float32(hi[0]), 0, 0, np.float32(1)])[0] for (_, p, lo, hi) in host]
    assert any(lo_hi)  # some two-corner boxes have min > max
    got = _inject(hip_ctx, g, records, lpv)
    want = _want(arrays, host, lpv)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), f"colour {c}: {int((got[c] != want[c]).sum())} halves differ"
    # a light lands in a neighbour cascade's cells: cascade 0's lights reach x >= 32 too
    assert np.count_nonzero(got[0][:, :, 32:]) > 0


@pytest.mark.parametrize("case", ["atrium", "soup"])
def test_injection_equals_per_cascade_inject_vpls(hip_ctx, case):
    import torch
    arrays = mesh.atrium().arrays() if case == "atrium" else _soup(40, (0.02, 0.15))  # every cascade's list within 4096
    view, sun, lpv = _lpv()
    g, records, host, keep = _clouds(hip_ctx, arrays, 3, lib.POINT_CLOUD_ON_SURFACE)
    got = _inject(hip_ctx, g, records, lpv)
    t = [util.to_torch(np.zeros(SHAPE, np.uint16)) for _ in range(3)]
    bounds = gml.cascade_bounds(lpv)
    for c in range(4):
        lists = [h[0] for h in host if len(h[0]) and gml.selected(arrays, h[1:], bounds[c])]
        if not lists:
            continue
        cat = np.concatenate(lists)
        assert len(cat) <= 4096
        lt = util.to_torch(np.ascontiguousarray(cat))
        cnt = util.to_torch(np.array([len(cat)], np.uint32))
        hip_ctx.lpv_inject_vpls(lt.data_ptr(), cnt.data_ptr(), len(cat), lpv.matrices, c, 4, [_vol(x) for x in t])
    torch.cuda.synchronize()
    ref = [util.from_torch(x, np.uint16).reshape(SHAPE) for x in t]
    for c in range(3):
        assert np.array_equal(got[c], ref[c]), f"colour {c}"


def _synthetic(n_clouds, points, hot, seed):
    """a scene of n_clouds SOLID emissive primitives (identity model, bounds covering every cascade) and random VPL lists around the
    camera; the first `hot` points of cloud 0 sit on one position (one cell per cascade takes them all)"""
    g = np.random.default_rng(seed)
    m = mesh.Mesh()
    mat = m.add_material(mesh.material(emission=(1.0, 1.0, 1.0, 0.0)))
    for _ in range(n_clouds):
        m.add_primitive([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1]] * 3, [0, 1, 2], mat)
    arrays = m.arrays()
    view, sun, lpv = _lpv()
    centre = np.array(view.position, np.float32)
    vp = []
    for k in range(n_clouds):
        pos = (centre + g.uniform(-30, 30, (points, 3))).astype(np.float16).view(np.uint16).astype(np.uint32)
        if k == 0:
            pos[:hot] = (centre + np.float32(0.3)).astype(np.float16).view(np.uint16).astype(np.uint32)
        col = g.uniform(0.001, 0.01, (points, 3)).astype(np.float16).view(np.uint16).astype(np.uint32)
        nrm = g.integers(-127, 128, (points, 3)) & 0xFF
        v = np.zeros((points, 4), np.uint32)
        v[:, 0] = pos[:, 0] | (pos[:, 1] << 16)
        v[:, 1] = pos[:, 2] | (col[:, 0] << 16)
        v[:, 2] = col[:, 1] | (col[:, 2] << 16)
        v[:, 3] = nrm[:, 0] | (nrm[:, 1] << 8) | (nrm[:, 2] << 16)
        vp.append(v)
    lo, hi = np.full(3, -1e6, np.float32), np.full(3, 1e6, np.float32)
    return arrays, lpv, vp, lo, hi


def _records(vp, lo, hi):
    ts = [util.to_torch(np.ascontiguousarray(v)) for v in vp]
    recs = [lib.EmissiveCloud(t.data_ptr(), len(v), k, (C.c_float * 3)(*lo.tolist()), (C.c_float * 3)(*hi.tolist())) for k, (t, v) in enumerate(zip(ts, vp))]
    return recs, ts


def test_a_million_entries_with_a_hot_cell_equals_numpy(hip_ctx):
    hot = 100000  # clouds 0, 1 and 2 on one position in cascade 0 (some of their lights are discarded: length(normalize(n)) < 1)
    arrays, lpv, vp, lo, hi = _synthetic(5, 60000, 60000, 17)
    vp[1][:, :2] = vp[0][0, :2]
    vp[2][:, :2] = vp[0][0, :2]
    g, keep = _device_scene(arrays)
    recs, ts = _records(vp, lo, hi)
    total = sum(len(v) for v in vp) * 4
    assert total >= 1_000_000
    got = _inject(hip_ctx, g, recs, lpv)
    host = [(v, k, lo, hi) for k, v in enumerate(vp)]
    cells, _ = gml.inject_terms(np.concatenate(vp), lpv.matrices[0], 0, 4, SHAPE[:3])
    assert np.bincount(cells[cells >= 0]).max() >= hot
    want = _want(arrays, host, lpv)
    for c in range(3):
        assert _same(got[c], want[c]), f"colour {c}: {int((got[c] != want[c]).sum())} halves differ"


def test_order_onto_filled_volumes_repeatability_and_capture(hip_ctx):
    import torch
    arrays = _soup()
    view, sun, lpv = _lpv()
    g, records, host, keep = _clouds(hip_ctx, arrays, 8, 0)
    rng = np.random.default_rng(2)
    prior = [rng.uniform(-2, 2, SHAPE).astype(np.float16).view(np.uint16) for _ in range(3)]
    got = _inject(hip_ctx, g, records, lpv, prior)
    want = _want(arrays, host, lpv, prior)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), f"colour {c}"
    assert [x.tobytes() for x in _inject(hip_ctx, g, records, lpv, prior)] == [x.tobytes() for x in got]
    # the call records under stream capture (no host synchronisation, no read-back) and the replay gives the same bytes
    t = [util.to_torch(v.copy()) for v in prior]
    with side_stream_context() as (ctx, s):
        with torch.cuda.stream(s):
            ctx.lpv_inject_emissive(g, records, lpv.matrices, lpv.bounds, 4, [_vol(x) for x in t])  # grows the scratch outside the capture
        s.synchronize()
        for x, v in zip(t, prior):
            x.copy_(util.to_torch(v.copy()))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ctx.lpv_inject_emissive(g, records, lpv.matrices, lpv.bounds, 4, [_vol(x) for x in t])
        graph.replay()
        torch.cuda.synchronize()
        for c in range(3):
            assert np.array_equal(util.from_torch(t[c], np.uint16).reshape(SHAPE), got[c])


def test_too_many_entries_is_refused(hip_ctx):
    arrays, lpv, vp, lo, hi = _synthetic(1, 4, 0, 3)
    g, keep = _device_scene(arrays)
    recs = [lib.EmissiveCloud(0x1000, (1 << 22) + 1, 0, (C.c_float * 3)(*lo.tolist()), (C.c_float * 3)(*hi.tolist()))]
    t = [util.to_torch(np.zeros(SHAPE, np.uint16)) for _ in range(3)]
    with pytest.raises(lib.SahError) as e:
        hip_ctx.lpv_inject_emissive(g, recs, lpv.matrices, lpv.bounds, 4, [_vol(x) for x in t])
    assert e.value.status == _abi.SAH_ERR_INVALID_ARGUMENT


# ---- an LPV frame with mesh lights -------------------------------------------------------------------------------------------------
def test_atrium_lpv_frame_with_mesh_lights(hip_ctx):
    """clear -> RSM / extract / inject -> mesh lights (on-surface clouds) -> propagate -> Lighting: the same frame as with the mesh-light
    step replaced by sah_lpv_inject_vpls on concatenated lists, and a lit image that differs from the frame without mesh lights"""
    import torch
    from tests.test_lpv_inject import _hip_rsm, _rsm_desc
    f = util.LightingFrame(160, 96, seed=61, sun_mode=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flavour="atrium")
    lpv, sun = f.lpv, f.sun
    arrays = mesh.atrium().arrays()
    rsm = _hip_rsm(hip_ctx, arrays, sun, lpv)
    desc = _rsm_desc(rsm)
    g, records, host, keep = _clouds(hip_ctx, arrays, 21, lib.POINT_CLOUD_ON_SURFACE)
    bounds = gml.cascade_bounds(lpv)
    images_out, volumes = {}, {}
    for mode in ("off", "mesh_lights", "inject_vpls"):
        a = [util.to_torch(np.full(SHAPE, 0x3C00, np.uint16)) for _ in range(3)]
        b = [torch.zeros_like(x) for x in a]
        hip_ctx.lpv_clear(*[_vol(x) for x in a], None, 4)
        vl = torch.zeros((4, 4096, 4), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
        for c in range(4):
            hip_ctx.lpv_extract_vpls(desc, lpv.matrices, c, 0.25, vl[c].data_ptr(), cnt[c:].data_ptr())
            hip_ctx.lpv_inject_vpls(vl[c].data_ptr(), cnt[c:].data_ptr(), 4096, lpv.matrices, c, 4, [_vol(x) for x in a])
        if mode == "mesh_lights":
            hip_ctx.lpv_inject_emissive(g, records, lpv.matrices, lpv.bounds, 4, [_vol(x) for x in a])
        elif mode == "inject_vpls":
            for c in range(4):
                lists = [h[0] for h in host if len(h[0]) and gml.selected(arrays, h[1:], bounds[c])]
                if lists:
                    cat = util.to_torch(np.ascontiguousarray(np.concatenate(lists)))
                    n = util.to_torch(np.array([len(cat)], np.uint32))
                    hip_ctx.lpv_inject_vpls(cat.data_ptr(), n.data_ptr(), len(cat), lpv.matrices, c, 4, [_vol(x) for x in a])
        hip_ctx.lpv_propagate([_vol(x) for x in a], [_vol(x) for x in b], 4, 4)
        torch.cuda.synchronize()
        volumes[mode] = [util.from_torch(x, np.uint16).reshape(SHAPE) for x in a]
        dev = f.device_arrays()
        for k, x in zip(("lpv_r", "lpv_g", "lpv_b"), a):
            dev[k] = x
        images_out[mode] = f.run_hip(hip_ctx, dev)
    for c in range(3):
        assert np.array_equal(volumes["mesh_lights"][c], volumes["inject_vpls"][c])
    assert np.array_equal(images_out["mesh_lights"], images_out["inject_vpls"])
    assert not np.array_equal(images_out["mesh_lights"], images_out["off"])
    lit = {k: v.view(np.float16)[..., :3].astype(np.float64) for k, v in images_out.items()}
    assert np.nansum(lit["mesh_lights"]) > np.nansum(lit["off"])  # the lamps add light
