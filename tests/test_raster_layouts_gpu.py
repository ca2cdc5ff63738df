"""The rasteriser's targets on pitched, offset images (tests/layouts.py) and its texture levels with padded rows: shadow cascades (the
dword and the half store of ShadowTarget::resolve, csrc/raster_tiles.hip), the five G-buffer planes, the three RSM volumes — bit-equal to the
oracle on tight arrays, bit-equal to the same library on tight images, every padding byte and every layer not rendered left as it was."""
import ctypes as C
import functools

import numpy as np
import pytest

from androidrenderer_amd import _abi, images, mesh, scene
from tests import layouts, util
from tests.layouts import D16, D32F, RGBA8, RGBA16F, SRGBA8
from tests.test_raster import _assert_gbuffers_equal, _oracle_gbuffer, _oracle_shadow, _ortho_sun, _quad, _soup_view

pytestmark = pytest.mark.gpu

OUT8, OUT16 = 0x07, 0x0707  # payload of a target before the call


def _geometry(arrays, pad_levels=False):
    """device geometry; with pad_levels every texture level has padded rows.  -> (descriptor, keep-alive list, wide texture arrays)"""
    dev = mesh.to_device(arrays)
    wides = []
    if pad_levels:
        dev["textures"], wides = layouts.pad_texture_levels(dev["textures"])
    keep = []
    return mesh.geometry(dev, keep), keep, wides


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- shadow cascades -----------------------------------------------------------------------------------------------------------------

def _shadow_spec(res, kind):
    """D16: base, row pitch and slice pitch must be even (csrc/api_raster.cpp: sah_shadow_render); two texels go out as one dword only when all
    three are multiples of 4.  Each of the first three kinds takes exactly one of them to 2 mod 4 and leaves the other two at multiples of 4."""
    row = 2 * res[0]
    if kind == "row_pitch_2_mod_4":    # the smallest padding that leaves the pitch at 2 mod 4: 2 or 4 bytes
        pad = 2 if row % 4 == 0 else 4
        return dict(row_pad=pad, slice_pad=(4 - res[1] * (row + pad) % 4) % 4)
    to4 = (4 - row % 4) % 4            # padding that brings the row pitch to a multiple of 4
    if kind == "base_2_mod_4":
        return dict(row_pad=to4 + 4, offset=2)
    if kind == "slice_pitch_2_mod_4":
        return dict(row_pad=to4 + 4, offset=4, slice_pad=2)
    assert kind == "multiples_of_4"
    return dict(row_pad=to4 + 8, offset=4, slice_pad=12)


SHADOW_KINDS = ["row_pitch_2_mod_4", "base_2_mod_4", "slice_pitch_2_mod_4", "multiples_of_4"]


def _hip_shadow(ctx, arrays, sun, cascades, res, spec, layers=None, pad_levels=False):
    import torch
    g, keep, wides = _geometry(arrays, pad_levels)
    layers = layers or cascades
    sm = layouts.pitched(torch.full((layers, res[1], res[0]), OUT16, dtype=torch.int16, device="cuda"), D16, 3, spec)
    stats = torch.zeros(_abi.RASTER_STATS_WORDS, dtype=torch.int32, device="cuda")
    ctx.shadow_render(g, sun, cascades, sm.volume(), stats.data_ptr())
    _sync()
    layouts.assert_padding_intact(sm, what="shadow_render")
    layouts.assert_texture_padding_intact(wides)
    return sm.read(np.uint16), sm


@functools.lru_cache(maxsize=None)
def _shadow_case(res):
    arrays = mesh.random_soup(3, triangles=600).arrays()
    view = _soup_view(320, 180, 3)
    sun = scene.DirectionalLight(shadow_mode=_abi.SHADOW_MODE_CSM)
    sun.set_direction([0.9, -1.0, 0.4])
    constants = sun.update_shadow_cascades(view, max_shadow_distance=32.0, resolution=res[0])
    want, _ = _oracle_shadow(arrays, constants, 4, res)
    assert (want != 0xffff).any()
    return arrays, constants, want


@pytest.mark.parametrize("kind", SHADOW_KINDS)
@pytest.mark.parametrize("res", [(65, 33), (66, 34)])
def test_shadow_render_half_and_dword_stores(hip_ctx, res, kind):
    """Every shadow test so far met the dword store of ShadowTarget::resolve.  A base, a row pitch or a slice pitch at 2 mod 4 must each switch
    it to the half stores on its own; four cascades, so that the slice pitch moves three of them."""
    arrays, constants, want = _shadow_case(res)
    spec = _shadow_spec(res, kind)
    got, sm = _hip_shadow(hip_ctx, arrays, constants, 4, res, spec)
    off4 = [name for name, v in (("base", sm.ptr), ("row_pitch", sm.row_pitch), ("slice_pitch", sm.slice_pitch)) if v % 4]
    assert off4 == {"multiples_of_4": []}.get(kind, [kind[:-len("_2_mod_4")]]), (kind, off4)  # the layout is the one the case names, and no other
    assert sm.row_pitch > 2 * res[0]
    tight, _ = _hip_shadow(hip_ctx, arrays, constants, 4, res, None)
    assert np.array_equal(got, want), f"{int((got != want).sum())} texels differ from the oracle"
    assert np.array_equal(got, tight)


@pytest.mark.parametrize("kind", ["row_pitch_2_mod_4", "multiples_of_4"])
def test_shadow_render_masked_soups_on_pitched_maps(hip_ctx, kind):
    """cut-outs in the shadow pass (the alpha test reads per-record attributes and, in the textured soup, the base colour texture): the masked
    quads of test_hip_masked_shadows_and_missing_attributes and the textured cut-out soup of test_textures, texture levels with padded rows"""
    m = mesh.Mesh()
    solid = m.add_material(mesh.material())
    leaf = m.add_material(mesh.material(opacity_threshold=0.5))
    _quad(m, 0, 8, 0, 8, 0.75, solid)
    _quad(m, 1, 4, 1, 4, 0.25, leaf, ptype=_abi.PRIMITIVE_TYPE_CUTOUT, colors=[0x20ffffff] * 4)
    _quad(m, 4, 7, 4, 7, 0.25, leaf, ptype=_abi.PRIMITIVE_TYPE_CUTOUT, colors=[0xffffffff] * 4)
    _quad(m, 0, 8, 5, 6, 0.10, leaf, ptype=_abi.PRIMITIVE_TYPE_CUTOUT, colors=[0x00ffffff, 0xffffffff, 0xffffffff, 0x00ffffff])
    want, _ = _oracle_shadow(m.arrays(), _ortho_sun(), 1, (8, 8))
    got, _ = _hip_shadow(hip_ctx, m.arrays(), _ortho_sun(), 1, (8, 8), _shadow_spec((8, 8), kind), layers=2)
    assert np.array_equal(got[0], want[0])
    assert (got[1] == OUT16).all()  # a layer beyond the cascades rendered
    # textured cut-outs
    arrays = mesh.random_soup(51, triangles=400, cutout_fraction=1.0, textured=True).arrays()
    sun = scene.DirectionalLight(shadow_mode=_abi.SHADOW_MODE_CSM)
    sun.update_shadow_cascades(scene.SceneView.default(320, 180), resolution=66)
    res = (66, 34)
    want, _ = _oracle_shadow(arrays, sun.constants, 4, res)
    assert (want != 0xffff).mean() > 0.02
    tight, _ = _hip_shadow(hip_ctx, arrays, sun.constants, 4, res, None)
    got, _ = _hip_shadow(hip_ctx, arrays, sun.constants, 4, res, _shadow_spec(res, kind), pad_levels=True)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got, tight)


# ---- G-buffer ---------------------------------------------------------------------------------------------------------------------------

GB_FORMATS = {"color": (SRGBA8, 2), "normals": (RGBA16F, 2), "data": (RGBA8, 2), "emission": (SRGBA8, 2), "depth": (D32F, 2)}
# base and pitch: multiples of 4, of 8 for the normals (csrc/api_raster.cpp: sah_gbuffer_render)
GB_LAYOUTS = {
    "A": {"color": dict(row_pad=4), "normals": dict(row_pad=8, offset=8), "data": dict(row_pad=4, offset=4), "emission": dict(row_pad=8, offset=4),
          "depth": dict(row_pad=4, offset=8)},
    "B": {"color": dict(row_pad=20, offset=4), "normals": dict(row_pad=24, offset=8), "data": dict(row_pad=12), "emission": dict(row_pad=28, offset=12),
          "depth": dict(row_pad=36, offset=4)},
}


def _hip_gbuffer(ctx, arrays, view, w, h, spec, pad_levels=False):
    import torch
    g, keep, wides = _geometry(arrays, pad_levels)
    out = {"color": torch.full((h, w, 4), OUT8, dtype=torch.uint8, device="cuda"), "normals": torch.full((h, w, 4), OUT16, dtype=torch.int16, device="cuda"),
           "data": torch.full((h, w, 4), OUT8, dtype=torch.uint8, device="cuda"), "emission": torch.full((h, w, 4), OUT8, dtype=torch.uint8, device="cuda"),
           "depth": torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")}
    p = layouts.wrap(out, GB_FORMATS, spec)
    gb = _abi.GBuffer(*[p[k].plane() for k in ("color", "normals", "data", "emission", "depth")])
    ctx.gbuffer_render(g, view.gpu_data, gb)
    _sync()
    layouts.assert_padding_intact(p, what="gbuffer_render")
    layouts.assert_texture_padding_intact(wides)
    return {k: p[k].read({"normals": np.uint16, "depth": np.float32}.get(k, np.uint8)) for k in p}


@pytest.mark.parametrize("layout", ["A", "B"])
@pytest.mark.parametrize("textured", [False, True])
def test_gbuffer_render_on_pitched_planes(hip_ctx, textured, layout):
    w, h = 129, 65
    arrays = mesh.random_soup(43 if textured else 12, triangles=500, textured=textured).arrays()
    view = scene.SceneView.default(w, h) if textured else _soup_view(w, h, 12)
    want, _ = _oracle_gbuffer(arrays, view, w, h)
    assert (want["depth"] > 0).mean() > 0.2
    tight = _hip_gbuffer(hip_ctx, arrays, view, w, h, None)
    got = _hip_gbuffer(hip_ctx, arrays, view, w, h, GB_LAYOUTS[layout])
    _assert_gbuffers_equal(got, want)
    _assert_gbuffers_equal(got, tight)


def test_texture_levels_with_padded_rows_in_the_gbuffer_pass(hip_ctx):
    """sah_texture levels carry a row pitch (csrc/texture_sample.hpp); mesh.geometry() takes it from the level's row stride.  The anisotropic
    golden scene (every material slot textured, four samplers, trilinear and anisotropic taps) from padded levels, from tight levels, and on the
    oracle — the same G-buffer; the targets are padded as well."""
    m, view = util.golden_raster_scene(anisotropic=True)
    arrays = m.arrays()
    want, _ = _oracle_gbuffer(arrays, view, 64, 36)
    flat, _ = _oracle_gbuffer(dict(arrays, textures=[]), view, 64, 36)
    assert not np.array_equal(flat["color"], want["color"])  # the textures do something
    tight = _hip_gbuffer(hip_ctx, arrays, view, 64, 36, None)
    got = _hip_gbuffer(hip_ctx, arrays, view, 64, 36, GB_LAYOUTS["B"], pad_levels=True)
    _assert_gbuffers_equal(got, want)
    _assert_gbuffers_equal(got, tight)


# ---- RSM ----------------------------------------------------------------------------------------------------------------------------------

RSM_FORMATS = {"flux": (SRGBA8, 3), "normals": (RGBA8, 3), "depth": (D16, 3)}
RSM_RES, RSM_LAYERS, RSM_CASCADES = 66, 4, 3
# texel-size multiples (csrc/api_raster.cpp: sah_rsm_render); the depth volume's row pitch is 2 * 66 + 2 = 134 or + 6 = 138: 2 mod 4 in both
RSM_LAYOUTS = {
    "A": {"flux": dict(row_pad=4, offset=4, slice_pad=4), "normals": dict(row_pad=8, slice_pad=4), "depth": dict(row_pad=2, offset=2, slice_pad=2)},
    "B": {"flux": dict(row_pad=20, offset=8, slice_pad=36), "normals": dict(row_pad=12, offset=4, slice_pad=100), "depth": dict(row_pad=6, slice_pad=50)},
}


def _hip_rsm(ctx, arrays, sun, lpv, spec):
    import torch
    g, keep, wides = _geometry(arrays)
    t = {"flux": torch.full((RSM_LAYERS, RSM_RES, RSM_RES, 4), OUT8, dtype=torch.uint8, device="cuda"),
         "normals": torch.full((RSM_LAYERS, RSM_RES, RSM_RES, 4), OUT8, dtype=torch.uint8, device="cuda"),
         "depth": torch.full((RSM_LAYERS, RSM_RES, RSM_RES), OUT16, dtype=torch.int16, device="cuda")}
    p = layouts.wrap(t, RSM_FORMATS, spec)
    ctx.rsm_render(g, sun.constants, lpv.matrices, RSM_CASCADES, _abi.RsmTargets(p["flux"].volume(), p["normals"].volume(), p["depth"].volume()))
    _sync()
    layouts.assert_padding_intact(p, what="rsm_render")
    return {k: p[k].read(np.uint16 if k == "depth" else np.uint8) for k in p}, p


@pytest.mark.parametrize("layout", ["A", "B"])
def test_rsm_render_on_pitched_volumes(hip_ctx, layout):
    """three cascades into volumes of four layers: the fourth keeps its payload"""
    from tests.test_lpv_inject import _setup
    _, sun, lpv = _setup()
    arrays = mesh.random_soup(31, triangles=800, extent=8.0).arrays()
    want = {"flux": np.zeros((RSM_CASCADES, RSM_RES, RSM_RES, 4), np.uint8), "normals": np.zeros((RSM_CASCADES, RSM_RES, RSM_RES, 4), np.uint8),
            "depth": np.zeros((RSM_CASCADES, RSM_RES, RSM_RES), np.uint16)}
    d = _abi.RsmTargets(images.volume(want["flux"], SRGBA8), images.volume(want["normals"], RGBA8), images.volume(want["depth"], D16))
    g = mesh.geometry(mesh.with_counts(arrays), [])
    assert util.oracle().orc_rsm_render(C.byref(g), C.byref(sun.constants), lpv.matrices, RSM_CASCADES, C.byref(d), None) == 0
    assert (want["depth"] != 0xffff).mean() > 0.2
    tight, _ = _hip_rsm(hip_ctx, arrays, sun, lpv, None)
    got, p = _hip_rsm(hip_ctx, arrays, sun, lpv, RSM_LAYOUTS[layout])
    assert p["depth"].row_pitch % 4 == 2
    for k in ("depth", "flux", "normals"):
        assert np.array_equal(got[k][:RSM_CASCADES], want[k]), f"rsm {k}: {int((got[k][:RSM_CASCADES] != want[k]).sum())} values differ from the oracle"
        assert (got[k][RSM_CASCADES:] == (OUT16 if k == "depth" else OUT8)).all(), f"rsm {k}: a layer beyond the cascades rendered was written"
        assert np.array_equal(got[k], tight[k])
