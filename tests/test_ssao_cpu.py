"""Screen-space ambient occlusion (include/sah_ssao.h) without a GPU: the export and the header, the 40-byte parameter block, the header's
two tables against the restatement's, every refusal the header lists, and the numpy restatement (tests/ssao_ref.py) — its committed fixture
with every planted case asserted to take its branch, that it is ambient occlusion on analytic scenes, and row windows."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib
from tests import ssao_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_ssao as gen  # noqa: E402

f32 = np.float32
D32, RGBA16F, R32F = _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R32_SFLOAT
HEADER = os.path.join(ROOT, "include", "sah_ssao.h")
FIELDS = ["radius", "max_radius_pixels", "shadow_multiplier", "shadow_clamp", "horizon_angle_threshold", "fade_out_from", "fade_out_to", "edge_sharpness",
          "blur_passes", "flags"]


# ---- exports, header, struct, tables --------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.SSAO_EXPORTS)
    header = open(HEADER).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.SSAO_EXPORTS) == ["sah_ssao"]
    assert not set(lib.SSAO_EXPORTS) & set(lib.EXPORTS)
    hip_h = open(os.path.join(ROOT, "include", "sah_hip.h")).read()
    assert "sah_ssao(" not in hip_h and re.search(r"#define\s+SAH_ABI_VERSION\s+6\b", hip_h)  # sah_hip.h's declarations and ABI version stay
    flat = " ".join(header.split())
    assert "ABI-defined" in header and "a pixel's value does not depend on the row window" in flat and "ANY row of `depth`" in flat


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles_and_the_parameter_block_is_40_bytes(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    offsets = "".join(f'{check}(offsetof(sah_ssao_params, {n}) == {4 * i}, "{n}");\n' for i, n in enumerate(FIELDS))
    src.write_text('#include <stddef.h>\n#include "sah_ssao.h"\n'
                   f'{check}(sizeof(sah_ssao_params) == 40, "sah_ssao_params");\n' + offsets +
                   "static const float offsets[SAH_SSAO_TAPS][2] = SAH_SSAO_OFFSETS;\nstatic const float rotations[16][2] = SAH_SSAO_ROTATIONS;\n"
                   "float first(void) { return offsets[0][0] + rotations[0][0]; }\n"
                   "int use(sah_ctx* c, const sah_view_data* v, const sah_plane* p, const sah_ssao_params* s) { return sah_ssao(c, v, p, p, p, p, s, 0, 0); }\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert C.sizeof(_abi.SsaoParams) == 40
    assert [(n, getattr(_abi.SsaoParams, n).offset) for n, _ in _abi.SsaoParams._fields_] == [(n, 4 * i) for i, n in enumerate(FIELDS)]
    d = _abi.SsaoParams.default()
    assert {n: getattr(d, n) for n in FIELDS} == {k: (f32(v) if isinstance(v, float) else v) for k, v in ref.DEFAULTS.items()}


def _header_table(name):
    body = re.search(r"#define " + name + r"\s*\\\n(.*?)\n\s*\}\n", open(HEADER).read(), re.S).group(1)
    values = [float.fromhex(v) for v in re.findall(r"(-?0x[0-9a-f.]+p[+-]\d+)f", body)]
    assert len(values) == 32
    table = np.array(values, np.float64).reshape(16, 2)
    assert (table.astype(f32).astype(np.float64) == table).all()  # exact fp32 values
    return table.astype(f32)


def test_the_headers_tables_are_the_restatements_bit_for_bit():
    off, rot = _header_table("SAH_SSAO_OFFSETS"), _header_table("SAH_SSAO_ROTATIONS")
    assert off.tobytes() == ref.offsets().tobytes() and rot.tobytes() == ref.rotations().tobytes()
    r = np.sqrt((off.astype(np.float64) ** 2).sum(-1))
    assert (r < 1).all() and np.abs(r - np.sqrt((np.arange(16) + 0.5) / 16)).max() < 1e-7  # in the unit disc, on the spiral
    norm = np.sqrt((rot.astype(np.float64) ** 2).sum(-1))
    assert np.abs(norm - 1).max() <= 2.0 ** -23
    assert len({tuple(v) for v in rot.tolist()}) == 16  # sixteen different rotations
    e = ref.rotated_offsets()
    assert e.shape == (16, 16, 2) and e.dtype == f32 and np.sqrt((e.astype(np.float64) ** 2).sum(-1)).max() < 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
OK, INVALID, FORMAT = "well-formed", _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
NAMES = ("depth", "normals", "scratch", "ao_out")
FORMATS = {"depth": D32, "normals": RGBA16F, "scratch": R32F, "ao_out": R32F}


def _plane(base, fmt, w, h, pitch=None, ptr=True, offset=0, bpp=None):
    bpp = _abi.FORMAT_BPP[fmt] if bpp is None else bpp
    return _abi.Plane((base + offset) if ptr else None, w, h, w * bpp if pitch is None else pitch, fmt)


def _view(changes=()):
    """a well-formed view; changes: {"z_near" or (matrix name, index): value}"""
    v = _abi.ViewData()
    for i in (0, 5, 10, 15):
        v.view[i] = 1.0
    v.projection[0], v.projection[5], v.projection[8], v.projection[9], v.z_near = 1.2, -2.0, 0.01, -0.02, 0.05
    for k, val in dict(changes).items():
        if k == "z_near":
            v.z_near = val
        else:
            getattr(v, k[0])[k[1]] = val
    return v


def _cases(base):
    """(name, [view, depth, normals, scratch, ao_out, params], rows, expected)"""
    W, H = 24, 16
    where = {n: base + (i << 16) for i, n in enumerate(NAMES)}

    def call(params=None, view=None, **kw):
        p = {n: _plane(where[n], FORMATS[n], W, H) for n in NAMES}
        p.update(kw)
        return [_view() if view is None else view] + [p[n] for n in NAMES] + [_abi.SsaoParams.default() if params is None else params]
    P = _abi.SsaoParams.default
    yield "whole", call(), (0, 0), OK
    yield "band", call(), (3, 9), OK
    yield "empty band", call(), (5, 5), OK
    for passes in (0, 1):
        yield f"blur_passes {passes}", call(P(blur_passes=passes)), (0, 0), OK
    yield "no blur, no scratch", call(P(blur_passes=0), scratch=None), (0, 0), OK
    yield "no blur, a scratch that is not looked at", call(P(blur_passes=0), scratch=_plane(where["scratch"], D32, 3, 0, ptr=False)), (0, 0), OK
    yield "no blur, scratch is ao_out's memory", call(P(blur_passes=0), scratch=_plane(where["ao_out"], R32F, W, H)), (0, 0), OK
    yield "padded pitches", call(depth=_plane(where["depth"], D32, W, H, pitch=W * 4 + 12), normals=_plane(where["normals"], RGBA16F, W, H, pitch=W * 8 + 4)), (0, 0), OK
    yield "limits of the ranges", call(P(max_radius_pixels=1.0, shadow_clamp=0.0, horizon_angle_threshold=1.0)), (0, 0), OK
    yield "limits of the ranges, other end", call(P(shadow_clamp=1.0, horizon_angle_threshold=0.0, max_radius_pixels=float("inf"))), (0, 0), OK
    yield "scratch NULL with a blur", call(scratch=None), (0, 0), INVALID
    yield "scratch NULL with one blur pass", call(P(blur_passes=1), scratch=None), (0, 0), INVALID
    yield "params NULL", call()[:5] + [None], (0, 0), INVALID
    yield "view NULL", [None] + call()[1:], (0, 0), INVALID
    for n in NAMES:
        fmt, bpp = FORMATS[n], _abi.FORMAT_BPP[FORMATS[n]]
        if n != "scratch":
            p = call()
            p[1 + NAMES.index(n)] = None
            yield f"{n}: null plane", p, (0, 0), INVALID
        yield f"{n}: null pointer", call(**{n: _plane(where[n], fmt, W, H, ptr=False)}), (0, 0), INVALID
        other = D32 if fmt != D32 else R32F
        yield f"{n}: wrong format", call(**{n: _plane(where[n], other, W, H, bpp=bpp)}), (0, 0), FORMAT
        yield f"{n}: short pitch", call(**{n: _plane(where[n], fmt, W, H, pitch=W * bpp - 4)}), (0, 0), INVALID
        yield f"{n}: zero width", call(**{n: _plane(where[n], fmt, 0, H)}), (0, 0), INVALID
        yield f"{n}: zero height", call(**{n: _plane(where[n], fmt, W, 0)}), (0, 0), INVALID
        yield f"{n}: other width", call(**{n: _plane(where[n], fmt, W - 1, H)}), (0, 0), INVALID
        yield f"{n}: other height", call(**{n: _plane(where[n], fmt, W, H + 1, pitch=W * bpp)}), (0, 0), INVALID
        yield f"{n}: misaligned pointer", call(**{n: _plane(where[n], fmt, W, H, offset=2)}), (0, 0), INVALID
        yield f"{n}: pitch not a multiple of 4", call(**{n: _plane(where[n], fmt, W, H, pitch=W * bpp + 2)}), (0, 0), INVALID
    yield "row_begin > row_end", call(), (9, 3), INVALID
    yield "row_end > H", call(), (0, H + 1), INVALID
    nan, inf = float("nan"), float("inf")
    for radius in (0.0, -1.0, inf, -inf, nan):
        yield f"radius {radius}", call(P(radius=radius)), (0, 0), INVALID
    for v in (0.999, 0.0, -3.0, nan):
        yield f"max_radius_pixels {v}", call(P(max_radius_pixels=v)), (0, 0), INVALID
    for field in ("shadow_clamp", "horizon_angle_threshold"):
        for v in (-0.001, 1.001, inf, -inf, nan):
            yield f"{field} {v}", call(P(**{field: v})), (0, 0), INVALID
    for lo, hi in ((50.0, 50.0), (300.0, 50.0), (nan, 300.0), (50.0, nan), (inf, inf)):
        yield f"fade {lo} .. {hi}", call(P(fade_out_from=lo, fade_out_to=hi)), (0, 0), INVALID
    for field in ("shadow_multiplier", "edge_sharpness"):
        yield f"{field} NaN", call(P(**{field: nan})), (0, 0), INVALID
    for passes in (3, 4, 0xffffffff):
        yield f"blur_passes {passes}", call(P(blur_passes=passes)), (0, 0), INVALID
    for flags in (1, 2, 0x80000000):
        yield f"flags {flags:#x}", call(P(flags=flags)), (0, 0), INVALID
    for key in [("projection", i) for i in (0, 5, 8, 9)] + [("view", i) for i in (0, 1, 2, 4, 5, 6, 8, 9, 10)] + ["z_near"]:
        yield f"NaN in {key}", call(view=_view({key: nan})), (0, 0), INVALID
    for key in [("projection", i) for i in (1, 2, 3, 4, 10, 14)] + [("view", i) for i in (3, 7, 12, 13, 14, 15)]:
        yield f"NaN in {key}, which is not read", call(view=_view({key: nan})), (0, 0), OK
    for z_near in (0.0, -0.05, inf):
        yield f"z_near {z_near}", call(view=_view({"z_near": z_near})), (0, 0), INVALID
    # the byte ranges of the two targets against the inputs' and each other's: the same plane, the last byte on the first, the first on the last
    size = {n: (H - 1) * W * _abi.FORMAT_BPP[FORMATS[n]] + W * _abi.FORMAT_BPP[FORMATS[n]] for n in NAMES}
    for target in ("ao_out", "scratch"):
        for n in [m for m in NAMES if m != target and not (target == "scratch" and m == "ao_out")]:
            yield f"{target} is {n}'s memory", call(**{target: _plane(where[n], R32F, W, H)}), (0, 0), INVALID
            yield f"{target} ends inside {n}", call(**{target: _plane(where[n] - size[target] + 4, R32F, W, H)}), (0, 0), INVALID
            yield f"{target} begins inside {n}", call(**{target: _plane(where[n] + size[n] - 4, R32F, W, H)}), (0, 0), INVALID
            yield f"{target} ends where {n} begins", call(**{target: _plane(where[n] - size[target], R32F, W, H)}), (0, 0), OK


def test_every_refusal_of_the_header_on_a_context_without_a_device():
    """A malformed call answers its status; a well-formed one gets as far as selecting the device, which a detached context does not have
    (SAH_ERR_HIP) — so nothing is launched and the made-up addresses are never used."""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present (made-up addresses must not reach a GPU); tests/test_ssao_gpu.py checks the refusals there")
    ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
    n = 0
    try:
        for name, args, rows, want in _cases(0x10000000):
            got = L.sah_ssao(h, *[ref_of(a) for a in args], *rows)
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"{name}: status {got}"
            n += 1
        ok = next(_cases(0x10000000))[1]
        assert L.sah_ssao(None, *[C.byref(a) for a in ok], 0, 0) == INVALID
    finally:
        L.sah_destroy(h)
    assert n > 120


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(gen.FIXTURE)


def test_generator_reproduces_the_committed_fixture(fixture):
    got = gen.generate(int(fixture["seed"]))
    assert sorted(got) == sorted(fixture.files)
    for k in fixture.files:
        assert np.asarray(got[k]).dtype == fixture[k].dtype and np.asarray(got[k]).tobytes() == fixture[k].tobytes(), k
    W, H = gen.WIDTH, gen.HEIGHT
    assert (W, H) == (69, 21) and all(W % t[0] and H % t[1] for t in (ref.RAW_TILE, ref.BLUR_TILE))  # a multiple of neither tile dimension
    assert fixture["depth_plane"].shape == (H, 72) and fixture["normals_plane"].shape == (H, 70, 4)   # padded pitches
    assert (fixture["depth_plane"][:, W:].view(np.uint32) == 0xA5A5A5A5).all() and (fixture["normals_plane"][:, W:] == 0xA5A5).all()
    assert os.path.getsize(gen.FIXTURE) < 160 * 1024


def test_every_planted_case_of_the_fixture_takes_its_branch(fixture):
    """The minimum counts are stated here; the generator's inputs are chosen so that the restatement alone meets them."""
    fx = fixture
    W, H = gen.WIDTH, gen.HEIGHT
    depth, normals = fx["depth_plane"][:, :W], fx["normals_plane"][:, :W]
    outs, infos = {}, {}
    for passes in (0, 1, 2):
        outs[passes], infos[passes] = ref.ssao_ex(depth, normals, gen.view(), dict(gen.PARAMS, blur_passes=passes))
        assert outs[passes].tobytes() == fx[f"ao_blur{passes}"].tobytes()
    assert (outs[0] != outs[1]).mean() > 0.3 and (outs[1] != outs[2]).mean() > 0.3
    info, raw = infos[2], outs[0]
    ok, live = info["centre_ok"], info["live"]
    # centres without a surface: sky, NaN, negative; with one at infinite depth (z = 0); all store 1.0
    assert (depth == 0).sum() >= 80 and np.isnan(depth).sum() == 6 and (depth < 0).sum() == 6 and np.isposinf(depth).sum() == 2
    assert not info["surface"][(depth == 0) | np.isnan(depth) | (depth < 0)].any() and (raw[~info["surface"]] == 1).all()
    assert info["surface"][np.isposinf(depth)].all()
    # zero and NaN normals on a surface: N is not finite, the pixel stores 1.0
    n16 = normals.view(np.float16)[..., :3]
    zero_n, nan_n = info["surface"] & (n16 == 0).all(-1), info["surface"] & np.isnan(n16).any(-1)
    assert zero_n.sum() >= 6 and nan_n.sum() >= 6 and not ok[zero_n | nan_n].any() and (raw[zero_n | nan_n] == 1).all()
    # the radius: clamped at 1, clamped at max_radius_pixels, and in between
    r_px, cap = info["r_px"], f32(gen.PARAMS["max_radius_pixels"])
    assert (live & (r_px == 1) & (info["t"] < 1)).sum() >= 300 and (live & (r_px == cap) & (info["t"] > cap)).sum() >= 300
    assert (live & (r_px > 1) & (r_px < cap)).sum() >= 200
    # taps outside the image on all four sides, taps on sky, a centre whose taps are all skipped
    assert {k: int(v.sum()) >= 20 for k, v in info["outside"].items()} == {"left": True, "right": True, "up": True, "down": True}
    assert info["on_sky"].sum() >= 100
    lone = ok & (info["count"] == 0)
    assert lone.sum() == 6 == len(gen.LONE) and all(lone[y, x] for x, y in gen.LONE) and (raw[lone] == 1).all()
    assert (ok & (info["count"] > 0) & (info["count"] < 16)).sum() >= 500 and (info["count"] == 16).sum() >= 30
    # the clamp of obs, and the three regimes of the fade
    floor = f32(1) - f32(gen.PARAMS["shadow_clamp"])
    assert info["clamped"].sum() >= 20 and (raw[info["clamped"]] == floor * np.sqrt(floor)).all() and (raw >= floor * np.sqrt(floor)).all()
    fade = info["fade"]
    assert (live & (fade == 0)).sum() >= 100 and (live & (fade == 1)).sum() >= 500 and (live & (fade > 0) & (fade < 1)).sum() >= 100
    assert (raw[live & (fade == 0)] == 1).all() and (raw[live & (fade > 0)] < 1).sum() >= 400
    # the blur, both passes: neighbours with weight 0, with weight 1, in between, without a surface; pixels on the image's border
    for b in info["blur"]:
        assert b["weight_zero"].sum() >= 500 and b["weight_one"].sum() >= 20 and b["weight_between"].sum() >= 300
        assert b["no_surface"].sum() >= 50 and b["border"].sum() == 2 * (W + H) - 4 - int((~info["surface"])[[0, -1]].sum() + (~info["surface"])[1:-1, [0, -1]].sum())
    assert np.isfinite(outs[2]).all() and (outs[2] <= 1).all() and (outs[2] > 0).all()


# ---- it is ambient occlusion ----------------------------------------------------------------------------------------------------------------
W, H = 96, 64
VIEW = ref.View.of(1.0, 1.5, 0.0, 0.0, 0.05)  # the identity view: world space is view space


def _padded_view(pad=0):
    """VIEW for an image widened by `pad` columns on either side: the same rays through the middle W columns, the same radius in pixels"""
    return VIEW if pad == 0 else ref.View.of(float(VIEW.p00) * W / (W + 2 * pad), 1.5, 0.0, 0.0, 0.05)


def _rays(pad=0):
    """(a, b): the point of pixel (x, y) at linear depth z is z * (a, b, -1)"""
    w, view = W + 2 * pad, _padded_view(pad)
    ndx = ((np.arange(w) + 0.5) * 2.0 / w - 1.0)[None, :] + np.zeros((H, 1))
    ndy = ((np.arange(H) + 0.5) * 2.0 / H - 1.0)[:, None] + np.zeros((1, w))
    return (ndx + float(view.p20)) / float(view.p00), (ndy + float(view.p21)) / float(view.p11)


def _plane_z(n, c, pad=0):
    """linear depth at which every pixel's ray meets the plane n . X = c (inf or negative where it does not, in front of the eye)"""
    a, b = _rays(pad)
    with np.errstate(divide="ignore"):
        return c / (n[0] * a + n[1] * b - n[2])


def _render(surfaces, concave=False, pad=0):
    """depth and normals of planes [(n, c)] with n facing the eye: the nearest hit (a convex solid's faces: the farthest), sky where no
    ray hits"""
    zs = np.stack([np.where(_plane_z(n, c, pad) > 0, _plane_z(n, c, pad), np.inf) for n, c in surfaces])
    pick = zs.argmin(0) if concave or len(surfaces) == 1 else np.where(np.isinf(zs), -np.inf, zs).argmax(0)
    z = np.take_along_axis(zs, pick[None], 0)[0]
    hit = np.isfinite(z) & (z > 0)
    depth = np.where(hit, float(VIEW.z_near) / np.where(hit, z, 1.0), 0.0).astype(f32)
    normals = np.zeros((H, W + 2 * pad, 4), np.float16)
    for i, (n, _) in enumerate(surfaces):
        normals[pick == i, :3] = np.array(n) * 1.7  # unnormalised, as the G-buffer's
    return depth, normals.view(np.uint16), z, pick


def _unit(v):
    return tuple(np.array(v, np.float64) / np.linalg.norm(v))


@pytest.mark.parametrize("normal", [(0.0, 0.0, 1.0), _unit((0.5, 0.2, 1.0)), _unit((-0.3, 0.4, 0.85))])
def test_a_flat_surface_is_unoccluded(normal):
    depth, normals, z, _ = _render([(normal, -6.0 * normal[2] - 0.5)])
    assert (depth > 0).all() and z.min() > 1
    for passes in (0, 2):
        ao, info = ref.ssao_ex(depth, normals, VIEW, dict(radius=2.0, blur_passes=passes))
        assert (ao == 1).all() and info["live"].all() and (info["r_px"] > 2).all()


def test_a_convex_edge_is_unoccluded():
    """two faces of a box seen from outside, the edge running down the middle of the image"""
    left, right = _unit((-0.5, 0.0, 1.0)), _unit((0.5, 0.0, 1.0))
    depth, normals, z, pick = _render([(left, -5.0 * left[2]), (right, -5.0 * right[2])])
    assert (depth > 0).all() and (pick[:, :W // 2] == 0).all() and (pick[:, W // 2:] == 1).all() and z[:, W // 2].max() < z[:, 0].min()  # the edge is nearest
    for passes in (0, 2):
        ao, info = ref.ssao_ex(depth, normals, VIEW, dict(radius=2.0, blur_passes=passes))
        assert (ao == 1).all() and info["live"].all() and (info["r_px"] > 4).all()


# a floor rising towards the eye below the middle of the image and a wall above it, at right angles, meeting in the line y = 0, z = -6
# (ndc y grows downwards: rows below the middle have y > 0)
_S = float(np.sqrt(0.5))
FLOOR, WALL = ((0.0, -_S, _S), -6.0 * _S), ((0.0, _S, _S), -6.0 * _S)
CREASE = H // 2  # the first floor row


def _crease(radius, passes, pad=0):
    depth, normals, z, pick = _render([WALL, FLOOR], concave=True, pad=pad)
    assert (pick[:CREASE] == 0).all() and (pick[CREASE:] == 1).all() and (depth > 0).all()
    ao, info = ref.ssao_ex(depth, normals, _padded_view(pad), dict(radius=radius, blur_passes=passes, max_radius_pixels=64.0))
    assert (info["r_px"] < 64).all() and (info["r_px"] > 4).all()
    a, b = _rays(pad)
    distance = np.hypot(z * b, 6.0 - z)  # of the pixel's point to the line y = 0, z = -6
    return ao, info, distance


def test_a_concave_crease_is_occluded_within_reach_and_nowhere_else():
    ao, info, distance = _crease(1.5, 0)
    assert (ao[CREASE - 1:CREASE + 1] < 1).all()  # strictly below 1 along the crease, on the wall's side and on the floor's
    # "farther than R": `distance` is fp64 from the analytic scene, R and the positions the pass works with are fp32, rounded a few times
    # at 6e-8 each, so a pixel counts as beyond only from R (1 + 1e-5) on; the band between is a hundredth of a pixel wide
    beyond = distance > info["R"].astype(np.float64) * (1 + 1e-5)
    assert beyond.sum() > 1000 and (ao[beyond] == 1).all() and (ao[~beyond] < 1).sum() > 500
    print(f"crease scene, radius 1.5, no blur: minimum {float(ao.min()):.4f}")


def _profile_pairs(blurred, info, distance):
    """(nearer row, farther row) pairs of neighbouring rows on one side of the crease, both wholly within reach of it"""
    within = distance < info["R"].astype(np.float64)
    floor_rows = [y for y in range(CREASE, H) if within[y].all()]
    wall_rows = [y for y in range(0, CREASE) if within[y].all()]
    assert len(floor_rows) >= 6 and len(wall_rows) >= 6
    return [(y - 1, y) for y in floor_rows[1:]] + [(y + 1, y) for y in wall_rows[:-1]]


def _eroded(mask, steps):
    """the pixels whose whole diamond of `steps` blur steps lies inside `mask` (and inside the image or beyond its edge)"""
    m = mask.copy()
    for _ in range(steps):
        n = m.copy()
        n[1:] &= m[:-1]
        n[:-1] &= m[1:]
        n[:, 1:] &= m[:, :-1]
        n[:, :-1] &= m[:, 1:]
        m = n
    return m


def _cross_max(a):
    """the maximum over a pixel and its four neighbours, those a blur pass reads"""
    m = a.copy()
    m[1:] = np.maximum(m[1:], a[:-1])
    m[:-1] = np.maximum(m[:-1], a[1:])
    m[:, 1:] = np.maximum(m[:, 1:], a[:, :-1])
    m[:, :-1] = np.maximum(m[:, :-1], a[:, 1:])
    return m


PAD = 20  # columns added on either side for the full-disc render: a multiple of 4 (the rotation pattern stays), r_px + 2 at least


def test_the_blurred_crease_is_non_increasing_towards_the_crease_pixel_by_pixel():
    """After two blur passes, over every pixel whose reach includes the crease: no pixel is brighter than its neighbour one row farther
    from the crease.  Left out, pixel by pixel, are only those whose reach the image cuts: a pixel with a tap of its own beyond a side of
    the image (the restatement's `outside` masks), and the pixels within the two steps over which the blur carries such a pixel's value.
    Over all 96 columns each row is strictly darker in the mean than the next one out.

    What the sides do is pinned against a render of the same scene PAD columns wider on either side, in which every one of the 96 columns
    has its whole disc: the pixels not left out equal it to rounding, so nothing but the cut changes a value; a pixel left out differs from
    it by no more than the cut can account for.  That bound is worked out, not measured: a pixel keeping n of its N taps, each worth at most
    o_max, moves its mean by at most o_max (N - n) / N, and x sqrt(x) has a slope of at most 1.5 on [0, 1]; a blur pass is a weighted mean
    with the same weights in both renders, so it passes on the largest difference among the five pixels it reads, and in the image's first
    and last column, where the wider render has a neighbour more, at weight 1 at most against the centre's 1, half the spread of those five
    values besides.  A pair of pixels can then be out of order by no more than the two bounds above what the full-disc render's pair is.

    Measured, and printed (DESIGN.md section 5q has the figures): of the 18 x 96 pixel pairs 22 are out of order, by 0.0264 at most, all
    within seven columns of a side, where 12 to 15 columns a side are left out; a pixel left out differs from the full-disc render by
    0.076 at most, against a bound of 0.69 at most.  The full-disc render itself has one pair out of order, by 0.0009, in a column this
    image leaves out: sixteen taps under a rotation that changes from pixel to pixel are an estimate, not a profile."""
    blurred, info, distance = _crease(1.5, 2)
    print(f"crease scene, radius 1.5, two blur passes: minimum {float(blurred.min()):.4f}, along the crease {float(blurred[CREASE - 1:CREASE + 1].max()):.4f} at most")
    assert (blurred[CREASE - 1:CREASE + 1] < 1).all()
    pairs = _profile_pairs(blurred, info, distance)
    rows = sorted({y for pair in pairs for y in pair})
    cut = np.logical_or.reduce(list(info["outside"].values()))
    assert not (info["outside"]["up"] | info["outside"]["down"])[rows].any()  # (in these rows only the image's sides cut a disc)
    whole = _eroded(~cut, 2)
    assert all(whole[y].sum() >= 64 for y in rows) and PAD % 4 == 0 and PAD >= info["r_px"][rows].max() + 2
    out_of_order = [(near, far, int(x)) for near, far in pairs for x in np.flatnonzero(blurred[near] > blurred[far])]
    worst = max([float(blurred[near, x] - blurred[far, x]) for near, far, x in out_of_order], default=0.0)
    print(f"  all columns: {len(out_of_order)} of {len(pairs) * W} pixel pairs out of order, by {worst:.4f} at most, columns "
          f"{sorted({x for _, _, x in out_of_order})}; left out per row: {sorted({int((~whole[y]).sum()) for y in rows})} of {W} pixels")
    for near, far in pairs:
        both = whole[near] & whole[far]
        assert (blurred[near, both] <= blurred[far, both]).all(), (near, far)
        assert blurred[near].astype(np.float64).mean() < blurred[far].astype(np.float64).mean(), (near, far)
    # the same scene with every disc whole
    middle = slice(PAD, PAD + W)
    wide_raw, wide_info, _ = _crease(1.5, 0, PAD)
    wide, _, _ = _crease(1.5, 2, PAD)
    assert not np.logical_or.reduce(list(wide_info["outside"].values()))[rows, PAD - 2:PAD + W + 2].any()  # (and the blur's two columns more)
    assert np.array_equal(wide_info["r_px"][:, middle], info["r_px"])
    difference = np.abs(blurred.astype(np.float64) - wide[:, middle])
    assert difference[whole].max() <= 1e-6  # (the rays of the two renders differ in their last bit)
    lost = wide_info["count"][:, middle] - info["count"]
    assert (lost >= 0).all() and (lost[rows] > 0).sum() > 300 and (lost[~cut] == 0).all()
    bound = 1.5 * wide_info["o_max"][:, middle].astype(np.float64) * lost / np.maximum(wide_info["count"][:, middle], 1) + 1e-6
    assert (np.abs(info["raw"].astype(np.float64) - wide_raw[:, middle]) <= bound).all()
    stage = wide_raw
    for _ in range(2):
        spread = (_cross_max(stage.astype(np.float64)) + _cross_max(-stage.astype(np.float64)))[:, middle]
        bound = _cross_max(bound)
        bound[:, [0, -1]] += 0.5 * spread[:, [0, -1]]
        stage = ref.blur_pass_ex(stage, _render([WALL, FLOOR], concave=True, pad=PAD)[0], VIEW.z_near, ref.DEFAULTS["edge_sharpness"])[0]
    assert np.array_equal(stage, wide)
    assert (difference <= bound).all(), [(y, x, difference[y, x], bound[y, x]) for y, x in np.argwhere(difference > bound)[:8]]
    print(f"  against the full-disc render: {difference[~whole & np.isin(np.arange(H), rows)[:, None]].max():.4f} at most on the pixels left out "
          f"(bound {bound[rows].max():.4f} at most); its own pairs out of order: "
          f"{[(near, far, int(x), round(float(wide[near, PAD + x] - wide[far, PAD + x]), 4)) for near, far in pairs for x in np.flatnonzero(wide[near, middle] > wide[far, middle])]}")
    for near, far, x in out_of_order:
        assert not (whole[near, x] and whole[far, x])
        assert blurred[near, x] - blurred[far, x] <= float(wide[near, PAD + x]) - float(wide[far, PAD + x]) + bound[near, x] + bound[far, x]


def test_halving_the_radius_never_darkens_a_pixel_outside_the_new_reach():
    full, _, _ = _crease(1.5, 0)
    half, info, distance = _crease(0.75, 0)
    outside = distance > info["R"].astype(np.float64) * (1 + 1e-5)  # (the fp32 slack of the test above)
    assert outside.sum() > 2000 and (half[outside] == 1).all() and (half[outside] >= full[outside]).all()
    assert (full[outside] < 1).sum() > 300  # (pixels the larger radius did darken)
    # blurred: a pass carries a value one pixel, so outside the new reach by more than two pixels
    full2, half2 = _crease(1.5, 2)[0], _crease(0.75, 2)[0]
    far = _eroded(outside, 2)
    assert far.sum() > 2000 and (half2[far] == 1).all() and (half2[far] >= full2[far]).all() and (full2[far] < 1).sum() > 300


def test_an_object_in_front_of_sky_takes_no_occlusion_from_the_sky():
    depth, normals, _, _ = _render([((0.0, 0.0, 1.0), -4.0)])
    yy, xx = np.mgrid[0:H, 0:W]
    sky = (np.hypot(xx - 48, yy - 32) > 22) | ((xx // 6 + yy // 6) % 5 == 0)  # a disc with holes
    depth = np.where(sky, f32(0), depth)
    for passes in (0, 2):
        ao, info = ref.ssao_ex(depth, normals, VIEW, dict(radius=2.0, blur_passes=passes))
        assert (ao == 1).all() and info["on_sky"].sum() > 500 and (info["live"] & (info["count"] < 16)).sum() > 500


# ---- row windows --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 2])
def test_three_bands_reassemble_the_whole_frame(fixture, passes):
    Wf, Hf = gen.WIDTH, gen.HEIGHT
    depth, normals = fixture["depth_plane"][:, :Wf], fixture["normals_plane"][:, :Wf]
    whole = fixture[f"ao_blur{passes}"]
    out = np.full((Hf, Wf), np.nan, f32)
    for rows in ((9, 10), (0, 9), (10, Hf)):
        band = ref.ssao(depth, normals, gen.view(), dict(gen.PARAMS, blur_passes=passes), rows)
        assert np.isnan(band[:rows[0]]).all() and np.isnan(band[rows[1]:]).all()
        out[rows[0]:rows[1]] = band[rows[0]:rows[1]]
        assert ref.band_rows(rows, Hf, passes) == (max(rows[0] - passes, 0), min(rows[1] + passes, Hf))
    assert out.tobytes() == whole.tobytes()
    assert np.isnan(ref.ssao(depth, normals, gen.view(), dict(gen.PARAMS, blur_passes=passes), (5, 5))).all() and ref.band_rows((5, 5), Hf, passes) == (5, 5)


# ---- the position route -------------------------------------------------------------------------------------------------------------------------
def test_positions_equal_the_inverse_projection_route_on_a_jittered_scene_view():
    """SceneView's projection (infinite reversed Z, jitter in column 2): z_near / depth and the two reciprocals give the view-space position
    the fp64 inverse of the projection gives, to fp32 rounding."""
    from androidrenderer_amd import scene
    from tests import mv_reproject
    w, h = 64, 36
    v = scene.SceneView.default(w, h)
    v.jitter = np.array([0.3, -0.2], f32)
    v.update_transforms()
    view = ref.View(v.gpu_data)
    assert view.p20 != 0 and view.p21 != 0
    depth = np.random.default_rng(3).uniform(0.0005, 0.9, (h, w)).astype(f32)
    surface, z = ref.linear_depth(depth, view.z_near)
    got = ref.positions(z, view, w, h).astype(np.float64)
    ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    ndc = np.stack([xs / (w * 0.5) - 1.0, ys / (h * 0.5) - 1.0, depth.astype(np.float64), np.ones((h, w))], -1)
    want = ndc @ np.linalg.inv(mv_reproject._m(v.gpu_data.projection)).T
    want = want[..., :3] / want[..., 3:4]
    assert surface.all() and np.abs(got - want).max() <= 1e-5 * np.abs(want).max(-1).max()
    assert (np.abs(got - want) <= 4e-6 * np.linalg.norm(want, axis=-1, keepdims=True)).all()
