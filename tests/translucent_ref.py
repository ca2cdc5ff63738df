"""Reference for sah_translucent_render (include/sah_translucent.h): a composition of what is already pinned, not a restatement.

For each translucent triangle in draw order the reference
  1. renders a G-buffer of that triangle alone as CUTOUT, with a copy of the material table whose opacity_threshold is -1 (no culling, no
     discard: the G-buffer pass's own vertex stage, clipping, fanning, snapping, fill rule, fragment depth and fragment stage),
  2. lights that G-buffer with the frame's Lighting descriptor and an AO plane of ones,
  3. takes the pixels where the layer's depth passes the strict test against the opaque depth and whose alpha code is not 0, and blends them
     in numpy: (S * a) + (D * (1 - a)) in fp32, every operator rounded, stored as a half.
Steps 1 and 2 run on a backend: the CPU oracle's rasteriser and lighting (OracleBackend), or sah_gbuffer_render + sah_lighting on the GPU
(HipBackend), which the rest of the suite pins to the oracle.  The scenes of the tests live here too, so that the CPU test, the fixture's
generator, the GPU tests and smoke() share them."""
import ctypes as C

import numpy as np

from androidrenderer_amd import _abi, images, mesh, synth
from tests import util

T = _abi.PRIMITIVE_TYPE_TRANSLUCENT
UNORM8 = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)  # the library's UNORM8-to-float table
GBUFFER_KEYS = ("color", "normals", "data", "emission", "depth")
GBUFFER_SHAPES = {"color": (4, np.uint8), "normals": (4, np.uint16), "data": (4, np.uint8), "emission": (4, np.uint8), "depth": (None, np.float32)}


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
# the camera of scene.SceneView.default is at (-7, 1, 0) and looks along +x; +z is to its right
def pane(m, x, y, z, mat, ptype=T, flip=False, **kw):
    """a rectangle at depth x facing the camera, y = (low, high), z = (left, right)"""
    pos = [(x, y[0], z[0]), (x, y[0], z[1]), (x, y[1], z[1]), (x, y[1], z[0])]
    uv = [(0.0, 0.0), (2.0, 0.0), (2.0, 1.5), (0.0, 1.5)]
    return m.add_primitive(pos, [(-1, 0, 0)] * 4, (0, 2, 1, 0, 3, 2) if flip else (0, 1, 2, 0, 2, 3), mat, ptype=ptype, texcoords=uv, **kw)


def glass(m, rgba, rough=0.3, metal=0.0, glow=(0, 0, 0, 0), **slots):
    """a material; glow: its emission factor; slots: texture indices by slot name"""
    return m.add_material(mesh.material(base=rgba, rough=rough, metal=metal, emission=glow), **slots)


def _alpha(codes):
    """vertex colours, white with the given alpha codes"""
    return np.array([0x00ffffff | (int(c) << 24) for c in codes], np.uint32)


def scene_panes(textured=True):
    """the atrium with glass in it, back to front: a far pane partly behind the columns, a textured one with random vertex colours, an
    emissive one that dips below the floor, a metallic one close to the camera, one against the sky above the end wall, one wholly behind
    the end wall, and a back-facing triangle.  Every pane glows a little, so that it shows under every sun mode and GI kind (with the sun off
    and no GI the lit image is the emission alone)"""
    g = synth.rng(771)
    m = mesh.atrium(1)
    tex = {}
    if textured:
        t0 = m.add_texture(*mesh.random_texture(g, 32, 32, None, True, mesh.sampler(), alpha=(40, 256)))
        t1 = m.add_texture(*mesh.random_texture(g, 16, 8, None, False, mesh.sampler(mag=0, min=1, mipmap=0, address_u=_abi.ADDRESS_MIRRORED_REPEAT)))
        t2 = m.add_texture(*mesh.random_texture(g, 8, 8, None, True, mesh.sampler(mag=1, min=0, mipmap=1)))
        tex = dict(base_color=t0, data=t1, emission=t2)
    pane(m, 16.0, (1.0, 9.0), (-4.0, 4.0), glass(m, (1.0, 1.0, 1.0, 0.9), glow=(0.2, 0.2, 0.2, 0.0)))  # behind the end wall: changes nothing
    pane(m, 10.0, (8.0, 16.0), (-4.0, 4.0), glass(m, (0.3, 0.5, 1.0, 0.6), glow=(0.05, 0.1, 0.3, 0.0)))  # against the sky above the end wall
    pane(m, 6.0, (0.0, 9.0), (-4.0, 4.0), glass(m, (1.0, 0.35, 0.3, 0.5), rough=0.6, glow=(0.3, 0.1, 0.05, 0.0)))  # far, the columns in front of it
    pane(m, 2.0, (0.5, 6.0), (-3.0, 1.5), glass(m, (0.9, 0.9, 0.9, 0.8), rough=0.5, metal=0.3, glow=(0.5, 0.4, 0.2, 0.0), **tex),
         colors=g.integers(0, 1 << 32, 4, dtype=np.uint64).astype(np.uint32) | np.uint32(0x50000000))
    pane(m, -1.0, (-0.5, 3.0), (-1.0, 3.5), glass(m, (0.4, 1.0, 0.5, 0.7), glow=(0.3, 1.0, 0.4, 0.0)))  # dips below the floor
    pane(m, -4.0, (0.2, 2.5), (-2.0, 0.5), glass(m, (0.8, 0.8, 1.0, 0.25), rough=0.15, metal=0.9, glow=(0.1, 0.1, 0.2, 0.0)))
    m.add_primitive([(-5.0, 1.5, 0.8), (-5.0, 1.5, 2.2), (-5.0, 2.6, 1.5)], [(-1, 0, 0)] * 3, (0, 2, 1), glass(m, (1.0, 0.9, 0.2, 0.55), glow=(0.3, 0.25, 0.0, 0.0)), ptype=T)  # back-facing
    return m


def scene_stack(layers=6, reverse=False):
    """`layers` panes one behind the other over part of the atrium's floor and far wall, each with its own colour and alpha"""
    m = mesh.Mesh()
    floor = m.add_material(mesh.material(base=(0.5, 0.45, 0.4, 1.0)))
    m.add_box((-14.5, -1.0, -5.0), (14.5, 0.0, 5.0), floor)
    order = list(range(layers))
    for k in (reversed(order) if reverse else order):
        x = -3.0 + 0.8 * (layers - 1 - k)  # k = 0 is the farthest; the nearest is 4 m from the camera
        rgba = (0.2 + 0.15 * k, 1.0 - 0.12 * k, 0.3 + 0.1 * (k % 3), 0.3 + 0.1 * k)
        pane(m, x, (-0.8 + 0.05 * k, 2.8), (-3.0 + 0.1 * k, 3.0), glass(m, rgba, rough=0.2 + 0.1 * k))
    return m


def scene_near():
    """a horizontal sheet of glass that runs through the camera plane (both of its triangles are clipped at the near plane and fanned) under
    the camera, a standing pane behind it and one in front of its far end"""
    m = mesh.Mesh()
    wall = m.add_material(mesh.material(base=(0.6, 0.5, 0.4, 1.0)))
    m.add_box((8.0, -3.0, -6.0), (9.0, 8.0, 6.0), wall)
    pane(m, 4.0, (-1.5, 2.5), (-2.5, 2.0), glass(m, (0.3, 0.6, 1.0, 0.5)))
    sheet = glass(m, (1.0, 0.8, 0.3, 0.6), rough=0.4)
    m.add_primitive([(-9.0, 0.2, -1.5), (6.0, 0.2, -1.5), (6.0, 0.2, 1.5), (-9.0, 0.2, 1.5)], [(0, 1, 0)] * 4, (0, 1, 2, 0, 2, 3), sheet, ptype=T,
                    colors=_alpha((255, 200, 140, 90)))
    pane(m, 1.0, (-0.5, 1.0), (-0.5, 2.5), glass(m, (0.9, 0.3, 0.6, 0.4)))
    return m


def scene_alpha_codes():
    """four panes side by side over a wall whose fragments carry the alpha codes 0, 1, 128 and 255"""
    m = mesh.Mesh()
    wall = m.add_material(mesh.material(base=(0.7, 0.6, 0.5, 1.0)))
    m.add_box((3.0, -6.0, -9.0), (4.0, 8.0, 9.0), wall)
    mat = glass(m, (0.2, 0.9, 0.4, 1.0))
    for i, code in enumerate((0, 1, 128, 255)):
        pane(m, -3.0, (-1.5, 3.5), (-4.4 + 2.2 * i, -2.4 + 2.2 * i), mat, colors=_alpha((code,) * 4))
    return m


def scene_long_list(triangles=300):
    """`triangles` small triangles of random depth, colour and alpha that all fall into the first 64 x 64 tile of a 96 x 54 frame: a bin
    list longer than one round of the tile kernel's walk"""
    g = synth.rng(772)
    m = mesh.Mesh()
    wall = m.add_material(mesh.material(base=(0.5, 0.5, 0.6, 1.0)))
    m.add_box((3.0, -6.0, -9.0), (4.0, 8.0, 9.0), wall)
    mat = glass(m, (1.0, 1.0, 1.0, 1.0), rough=0.5)
    centre = np.stack([g.uniform(-2.5, -1.5, triangles), g.uniform(-2.0, 4.0, triangles), g.uniform(-5.5, 0.5, triangles)], axis=1)
    pos = (centre[:, None, :] + np.concatenate([np.zeros((triangles, 3, 1)), g.uniform(-0.7, 0.7, (triangles, 3, 2))], axis=2)).reshape(-1, 3)
    col = g.integers(0, 1 << 32, 3 * triangles, dtype=np.uint64).astype(np.uint32) | np.uint32(0x30000000)
    m.add_primitive(pos.astype(np.float32), [(-1, 0, 0)] * (3 * triangles), np.arange(3 * triangles), mat, ptype=T, colors=col)
    return m


# ---- backends -----------------------------------------------------------------------------------------------------------------------------
def new_gbuffer(w, h):
    return {k: np.zeros((h, w) + ((c,) if c else ()), dt) for k, (c, dt) in GBUFFER_SHAPES.items()}


class OracleBackend:
    """steps 1 and 2 on the CPU oracle"""

    def gbuffer(self, arrays, view, w, h):
        out = new_gbuffer(w, h)
        g = mesh.geometry(mesh.with_counts(arrays), [])
        gb = images.gbuffer(out)
        assert util.oracle().orc_gbuffer_render(C.byref(g), C.byref(view.gpu_data), C.byref(gb), None) == 0
        return out

    def lighting(self, f, gb, rows=(0, 0)):
        arrays = dict(f.arrays)
        arrays.update(gb)
        arrays["ao"] = np.ones((f.height, f.width), np.float32)
        lit = np.zeros((f.height, f.width, 4), np.uint16)
        f.row_begin, f.row_end = rows
        try:
            d, keep = f.describe(arrays, lit)
        finally:
            f.row_begin = f.row_end = 0
        assert util.oracle().orc_lighting(C.byref(d)) == 0
        return lit


class HipBackend:
    """steps 1 and 2 on the GPU: sah_gbuffer_render and sah_lighting"""

    def __init__(self, ctx):
        self.ctx = ctx
        self._dev = {}

    def _scene(self, arrays):
        key = id(arrays["positions"])
        if key not in self._dev:
            self._dev[key] = (arrays["positions"], mesh.to_device(arrays))
        return self._dev[key][1]

    def gbuffer(self, arrays, view, w, h):
        import torch
        dev = dict(self._scene(arrays))
        for k in ("primitives", "materials"):  # (a layer differs from the scene in these two alone)
            dev[k] = util.to_torch(np.frombuffer(np.ascontiguousarray(arrays[k]).tobytes(), np.uint8).copy())
        dev["counts"] = mesh.with_counts(arrays)["counts"]
        out = {k: torch.zeros((h, w) + ((c,) if c else ()), dtype={np.uint8: torch.uint8, np.uint16: torch.int16, np.float32: torch.float32}[dt], device="cuda")
               for k, (c, dt) in GBUFFER_SHAPES.items()}
        self.ctx.gbuffer_render(mesh.geometry(dev, []), view.gpu_data, images.gbuffer(out))
        torch.cuda.synchronize()
        return {k: util.from_torch(v, GBUFFER_SHAPES[k][1]) for k, v in out.items()}

    def lighting(self, f, gb, rows=(0, 0)):
        import torch
        key = ("frame", id(f))
        if key not in self._dev:
            self._dev[key] = (f, f.device_arrays())
        dev = dict(self._dev[key][1])
        for k in GBUFFER_KEYS:
            dev[k] = util.to_torch(np.ascontiguousarray(gb[k]))
        dev["ao"] = torch.ones((f.height, f.width), dtype=torch.float32, device="cuda")
        lit = torch.zeros((f.height, f.width, 4), dtype=torch.int16, device="cuda")
        f.row_begin, f.row_end = rows
        try:
            d, keep = f.describe(dev, lit)
        finally:
            f.row_begin = f.row_end = 0
        self.ctx.lighting(d)
        torch.cuda.synchronize()
        return util.from_torch(lit, np.uint16)


# ---- the composition ----------------------------------------------------------------------------------------------------------------------
def single_triangle_records(translucent):
    """one primitive record per triangle of `translucent` (the translucent half of a split scene), in draw order: the primitive's own record
    narrowed to that triangle's three indices, as CUTOUT"""
    out = []
    for p in translucent["primitives"]:
        for tri in range(int(p["index_count"]) // 3):
            r = p.copy()
            r["first_index"], r["index_count"], r["type"] = int(p["first_index"]) + 3 * tri, 3, _abi.PRIMITIVE_TYPE_CUTOUT
            out.append(r)
    return np.array(out, dtype=mesh.PRIMITIVE) if out else np.zeros(0, mesh.PRIMITIVE)


def blend(dst_bits, src_bits, code):
    """(S * a) + (D * (1 - a)) per channel in fp32, every operator rounded, stored as halfs; code: the fragment's alpha code per pixel"""
    a = UNORM8[code][..., None]
    s, d = src_bits.view(np.float16).astype(np.float32), dst_bits.view(np.float16).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((s * a) + (d * (np.float32(1.0) - a))).astype(np.float16).view(np.uint16)


class Frame:
    """One frame with translucent geometry: `m` a mesh.Mesh (or its arrays) whose type-2 primitives are in back-to-front order.  The opaque
    half is rasterised into the G-buffer of a util.LightingFrame (synthetic shadow cascades, LPV volumes and sky), which Lighting turns into
    `lit0`, the image the translucent pass starts from; `compose` is the reference for what it must end with."""

    def __init__(self, backend, m, w, h, sun=_abi.SHADOW_MODE_CSM, gi=_abi.GI_LPV, flags=_abi.LIGHTING_DEFAULT_FLAGS, sky=True, seed=61):
        self.backend, self.w, self.h = backend, w, h
        self.arrays = m.arrays() if hasattr(m, "arrays") else m
        self.opaque, self.translucent = mesh.split_translucent(self.arrays)
        self.f = util.LightingFrame(w, h, gbuffer=new_gbuffer(w, h), seed=seed, sun_mode=sun, gi=gi, sky=sky, flags=flags, shadowmap_res=64)
        self.f.arrays.update(backend.gbuffer(self.opaque, self.f.view, w, h))
        self.depth = self.f.arrays["depth"]
        # the frame's own Lighting pass, with the frame's AO plane (a layer is lit with an AO of 1 instead)
        self.lit0 = self.f.run_oracle() if isinstance(backend, OracleBackend) else self.f.run_hip(backend.ctx)
        self.lit0.setflags(write=False)

    def compose(self, translucent=None, rows=(0, 0)):
        """(lit, blended): the image after the translucent pass and, per pixel, how many fragments were blended"""
        translucent = self.translucent if translucent is None else translucent
        r0, r1 = (0, self.h) if tuple(rows) == (0, 0) else rows
        lit = np.array(self.lit0)
        blended = np.zeros((self.h, self.w), np.int32)
        materials = translucent["materials"].copy()
        materials["opacity_threshold"] = -1.0
        in_rows = np.zeros((self.h, self.w), bool)
        in_rows[r0:r1] = True
        records = single_triangle_records(translucent)
        for i in range(len(records)):
            layer = dict(translucent, primitives=records[i:i + 1], materials=materials)
            gb = self.backend.gbuffer(layer, self.f.view, self.w, self.h)
            with np.errstate(invalid="ignore"):
                take = (gb["depth"] > self.depth) & in_rows & (gb["color"][..., 3] != 0)
            if not take.any():
                continue
            src = self.backend.lighting(self.f, gb)
            out = blend(lit, src, gb["color"][..., 3])
            lit[take] = out[take]
            blended += take
        return lit, blended


def assert_preconditions(fr, want, blended, min_changed=0.2, min_depth=1):
    """a degenerate scene must not pass quietly: enough pixels change, some pixel is deep enough"""
    changed = (want != fr.lit0).any(-1)
    assert changed.mean() >= min_changed, f"only {changed.mean():.3f} of the pixels change"
    assert blended.max() >= min_depth, f"the deepest pixel blends {blended.max()} fragments, fewer than {min_depth}"
    assert not ((want & 0x7fff) > 0x7c00).any(), "a NaN in the reference image: payloads are not part of the contract"
