"""Volumetric sun light (include/sah_sun_shafts.h) without a GPU: the export and the header, the 60-byte structure and its defaults, every
refusal the header lists on a context without a device, an argument fuzz in a child process, and the numpy restatement
(tests/sun_shafts_ref.py) — the properties the design rests on and its committed fixture."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib
from tests import sun_shafts_ref as ref
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_sun_shafts as gen  # noqa: E402

f32 = np.float32
HEADER = os.path.join(ROOT, "include", "sah_sun_shafts.h")
PARAM_OFFSETS = [("step_length", 0), ("num_steps", 4), ("step_transmittance", 8), ("albedo", 12), ("ambient", 24), ("anisotropy", 36), ("depth_bias", 40),
                 ("depth_sharpness", 44), ("downscale", 48), ("dither_offset", 52), ("flags", 56)]
RGBA16, D32, D16 = _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_D16_UNORM
FORMATS = dict(depth=D32, lit=RGBA16, march=RGBA16, out=RGBA16)
ORDER = ("depth", "lit", "march", "out")


# ---- exports, header, structure -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.SUN_SHAFTS_EXPORTS)
    header = open(HEADER).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.SUN_SHAFTS_EXPORTS) == ["sah_sun_shafts"]
    assert not set(lib.SUN_SHAFTS_EXPORTS) & set(lib.EXPORTS)
    hip_h = open(os.path.join(ROOT, "include", "sah_hip.h")).read()
    assert "sah_sun_shafts" not in hip_h and re.search(r"#define\s+SAH_ABI_VERSION\s+6\b", hip_h)  # sah_hip.h's declarations and ABI version stay
    assert "ABI-defined" in header and "Parity unpinned" in header and "Off by default" in header
    assert re.search(r"#define\s+SAH_SUN_SHAFTS_DITHER\s+1u\b", header) and re.search(r"#define\s+SAH_SUN_SHAFTS_TERM_ONLY\s+2u\b", header)
    assert re.search(r"#define\s+SAH_SUN_SHAFTS_MAX_STEPS\s+64u\b", header)
    assert (_abi.SUN_SHAFTS_DITHER, _abi.SUN_SHAFTS_TERM_ONLY) == (ref.DITHER, ref.TERM_ONLY) == (1, 2) and lib.SUN_SHAFTS_MAX_STEPS == ref.MAX_STEPS == 64


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles_and_the_structure_is_60_bytes(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    offsets = "".join(f'{check}(offsetof(sah_sun_shafts_params, {n}) == {o}, "{n}");\n' for n, o in PARAM_OFFSETS)
    src.write_text('#include <stddef.h>\n#include "sah_sun_shafts.h"\n'
                   f'{check}(sizeof(sah_sun_shafts_params) == 60, "sah_sun_shafts_params");\n' + offsets +
                   "int use(sah_ctx* c, const sah_view_data* v, const sah_sun_light_constants* s, const sah_volume* m, const sah_plane* p, const sah_sun_shafts_params* q) {\n"
                   "    return sah_sun_shafts(c, v, s, m, p, p, p, p, q, 0, 0) + (int)SAH_SUN_SHAFTS_DITHER + (int)SAH_SUN_SHAFTS_TERM_ONLY; }\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert C.sizeof(_abi.SunShaftsParams) == 60
    assert [(n, getattr(_abi.SunShaftsParams, n).offset) for n, _ in _abi.SunShaftsParams._fields_] == PARAM_OFFSETS


def test_the_headers_defaults_are_the_python_defaults():
    header = open(HEADER).read()
    d = _abi.SunShaftsParams.default()
    for name in ("step_length", "num_steps", "step_transmittance", "albedo", "ambient", "anisotropy", "depth_bias", "depth_sharpness", "downscale",
                 "dither_offset", "flags"):
        m = re.search(rf"#define\s+SAH_SUN_SHAFTS_DEFAULT_{name.upper()}\s+([0-9.]+)[fu]\b", header)
        assert m, name
        mine, restated = getattr(d, name), ref.DEFAULTS[name]
        if name in ("albedo", "ambient"):
            assert len(set(mine)) == len(set(restated)) == 1
            mine, restated = mine[0], restated[0]
        assert f32(float(m.group(1))) == f32(mine) == f32(restated), name
        text = m.group(1).rstrip("0").rstrip(".") if "." in m.group(1) else m.group(1)
        assert re.search(rf"\b{name}(\[3\])?;(?:(?!\*/).)*?default {re.escape(text)} \*/", header, re.S), name  # the field's comment says the same
    changed = _abi.SunShaftsParams.default(num_steps=7, ambient=(0.25, 0.5, 1.0), flags=3)
    assert (changed.num_steps, tuple(changed.ambient), changed.flags, changed.step_length) == (7, (0.25, 0.5, 1.0), 3, 0.5)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
OK, INVALID, FORMAT = "well-formed", _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT
W, H = 40, 23
EXTENT = dict(depth=(W, H), lit=(W, H), out=(W, H), march=(W, H))
HALF = (20, 12)


def _plane(name, base, w=None, h=None, pitch=None, ptr=True, offset=0, fmt=None):
    bpp = _abi.FORMAT_BPP[FORMATS[name]]
    w = EXTENT[name][0] if w is None else w
    h = EXTENT[name][1] if h is None else h
    return _abi.Plane((base + offset) if ptr else None, w, h, w * bpp if pitch is None else pitch, FORMATS[name] if fmt is None else fmt)


def _volume(base, w=64, h=64, layers=4, fmt=D16, row_pitch=None, slice_pitch=None, ptr=True, offset=0):
    bpp = _abi.FORMAT_BPP.get(fmt, 2)
    row_pitch = w * bpp if row_pitch is None else row_pitch
    return _abi.Volume((base + offset) if ptr else None, w, h, layers, row_pitch, row_pitch * h if slice_pitch is None else slice_pitch, fmt)


def _cases(base):
    """(name, (view, sun, shadowmap, planes by name, params, row_begin, row_end), expected)"""
    at = {n: base + (i << 16) for i, n in enumerate(ORDER)}
    at_map = base + (8 << 16)
    P = _abi.SunShaftsParams.default
    size8 = (H - 1) * W * 8 + W * 8
    view, sun = _abi.ViewData(), _abi.SunLightConstants()
    view.z_near = 0.05

    def call(rows=(0, 0), params="default", view=view, sun=sun, shadowmap="default", **kw):
        planes = {n: _plane(n, at[n]) for n in ORDER}
        planes.update(kw)
        return (view, sun, _volume(at_map) if shadowmap == "default" else shadowmap, planes, P() if params == "default" else params) + tuple(rows)

    def half(**kw):
        planes = dict(march=_plane("march", at["march"], *HALF))
        planes.update(kw)
        return planes
    yield "whole", call(), OK
    yield "band", call((3, 9)), OK
    yield "empty band", call((5, 5)), OK
    yield "last row", call((H - 1, H)), OK
    yield "downscale 2", call(params=P(downscale=2), **half()), OK
    yield "no shadow map", call(shadowmap=None), OK
    yield "a shadow map without memory", call(shadowmap=_volume(at_map, ptr=False)), OK
    yield "one D32 layer", call(shadowmap=_volume(at_map, 8, 8, 1, D32)), OK
    yield "nine layers", call(shadowmap=_volume(at_map, layers=9)), OK
    yield "a padded shadow map", call(shadowmap=_volume(at_map, row_pitch=64 * 2 + 6, slice_pitch=(64 * 2 + 6) * 64 + 10)), OK
    yield "term only without lit", call(params=P(flags=2), lit=None), OK
    yield "term only ignores lit", call(params=P(flags=3), lit=_plane("lit", at["lit"], fmt=D32, w=3)), OK
    yield "padded pitches", call(lit=_plane("lit", at["lit"], pitch=W * 8 + 12), out=_plane("out", at["out"], pitch=W * 8 + 4),
                                 march=_plane("march", at["march"], pitch=W * 8 + 8)), OK
    yield "limits of the ranges", call(params=P(step_length=1e-30, num_steps=1, step_transmittance=1.0, anisotropy=0.999, depth_sharpness=0.0, dither_offset=15, flags=3)), OK
    yield "other limits", call(params=P(step_length=3e38, num_steps=64, step_transmittance=1e-30, albedo=(3e38, -3e38, 0.0), ambient=(-3e38, 3e38, 0.0),
                                        anisotropy=-0.999, depth_bias=-3e38, depth_sharpness=3e38)), OK
    yield "out ends where lit begins", call(out=_plane("out", at["lit"] - size8)), OK
    yield "view NULL", call(view=None), INVALID
    yield "sun NULL", call(sun=None), INVALID
    yield "params NULL", call(params=None), INVALID
    for name in ORDER:
        yield f"{name} NULL", call(**{name: None}), INVALID
        yield f"{name}: null pointer", call(**{name: _plane(name, at[name], ptr=False)}), INVALID
        yield f"{name}: wrong format", call(**{name: _plane(name, at[name], fmt=_abi.FORMAT_R32_SFLOAT)}), FORMAT
        bpp = _abi.FORMAT_BPP[FORMATS[name]]
        yield f"{name}: short pitch", call(**{name: _plane(name, at[name], pitch=W * bpp - 4)}), INVALID
        yield f"{name}: misaligned pointer", call(**{name: _plane(name, at[name], offset=2)}), INVALID
        yield f"{name}: pitch not a multiple of 4", call(**{name: _plane(name, at[name], pitch=W * bpp + 2)}), INVALID
        yield f"{name}: zero width", call(**{name: _plane(name, at[name], w=0)}), INVALID
        yield f"{name}: zero height", call(**{name: _plane(name, at[name], h=0)}), INVALID
        yield f"{name}: other width", call(**{name: _plane(name, at[name], w=W + 1, pitch=(W + 1) * bpp)}), INVALID
        yield f"{name}: other height", call(**{name: _plane(name, at[name], h=H - 1)}), INVALID
    yield "march of the half grid under downscale 1", call(**half()), INVALID
    yield "march of the frame's extent under downscale 2", call(params=P(downscale=2)), INVALID
    yield "march of the floor, not the ceiling", call(params=P(downscale=2), march=_plane("march", at["march"], 20, 11)), INVALID
    big = {n: _plane(n, at[n], w=65536, h=65536) for n in ORDER}  # (a pitch of 2^19 bytes still fits its field)
    yield "2^32 texels", call(**big), INVALID
    yield "2^32 texels under downscale 2", call(params=P(downscale=2), **dict(big, march=_plane("march", at["march"], w=32768, h=32768))), INVALID
    yield "one texel fewer than 2^32 is a matter of memory, not of the header", call(**{n: _plane(n, at[n] + (i << 44), w=65535, h=65536) for i, n in enumerate(ORDER)}), OK  # (32 GiB planes, set apart)
    yield "row_begin > row_end", call((9, 3)), INVALID
    yield "row_end > h", call((0, H + 1)), INVALID
    yield "shadow map: wrong format", call(shadowmap=_volume(at_map, fmt=RGBA16)), FORMAT
    yield "shadow map: no layer", call(shadowmap=_volume(at_map, layers=0)), INVALID
    yield "shadow map: zero width", call(shadowmap=_volume(at_map, w=0)), INVALID
    yield "shadow map: zero height", call(shadowmap=_volume(at_map, h=0)), INVALID
    yield "shadow map: short row pitch", call(shadowmap=_volume(at_map, row_pitch=64 * 2 - 2, slice_pitch=64 * 64 * 2)), INVALID
    yield "shadow map: short slice pitch", call(shadowmap=_volume(at_map, slice_pitch=64 * 64 * 2 - 2)), INVALID
    yield "shadow map: misaligned pointer", call(shadowmap=_volume(at_map, offset=1)), INVALID
    yield "shadow map: D32 on a 2-byte boundary", call(shadowmap=_volume(at_map, fmt=D32, offset=2)), INVALID
    yield "shadow map: odd row pitch", call(shadowmap=_volume(at_map, row_pitch=64 * 2 + 1, slice_pitch=(64 * 2 + 1) * 64 + 1)), INVALID
    yield "shadow map: a layer of 4 GiB", call(shadowmap=_volume(at_map, w=32768, h=65536, fmt=D16)), INVALID
    nan, inf = float("nan"), float("inf")
    bad = dict(step_length=(0.0, -0.5, inf, nan), num_steps=(0, 65, 0xFFFFFFFF), step_transmittance=(0.0, -0.5, 1.001, inf, nan), anisotropy=(1.0, -1.0, 1.5, inf, nan),
               depth_bias=(inf, -inf, nan), depth_sharpness=(-0.001, inf, nan), downscale=(0, 3, 4, 0xFFFFFFFF), dither_offset=(16, 0xFFFFFFFF),
               flags=(4, 7, 0x80000000))
    for field, values in bad.items():
        for v in values:
            yield f"{field} {v}", call(params=P(**{field: v})), INVALID
    for field in ("albedo", "ambient"):
        for v in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf)):
            yield f"{field} {v}", call(params=P(**{field: v})), INVALID
    for z_near in (0.0, -0.05, inf, nan):
        other = _abi.ViewData()
        other.z_near = z_near
        yield f"z_near {z_near}", call(view=other), INVALID
    # overlaps
    for name in ORDER[:-1]:
        yield f"out is {name}'s memory", call(out=_plane("out", at[name])), INVALID
    yield "out ends inside lit", call(out=_plane("out", at["lit"] - size8 + 4)), INVALID
    yield "out begins inside lit", call(out=_plane("out", at["lit"] + size8 - 4)), INVALID
    for name in ORDER[:2]:
        yield f"march is {name}'s memory", call(march=_plane("march", at[name])), INVALID


def _invoke(L, h, args):
    view, sun, shadowmap, planes, params, r0, r1 = args
    ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
    return L.sah_sun_shafts(h, ref_of(view), ref_of(sun), ref_of(shadowmap), *[ref_of(planes[n]) for n in ORDER], ref_of(params), r0, r1)


def test_every_refusal_of_the_header_on_a_context_without_a_device():
    """A malformed call answers its status; a well-formed one gets as far as selecting the device, which a detached context does not have
    (SAH_ERR_HIP) — so nothing is launched and the made-up addresses are never used."""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present (made-up addresses must not reach a GPU); tests/test_sun_shafts_gpu.py checks the refusals there")
    n = 0
    try:
        for name, args, want in _cases(0x10000000):
            got = _invoke(L, h, args)
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"{name}: status {got}"
            n += 1
        assert _invoke(L, None, next(_cases(0x10000000))[1]) == INVALID
    finally:
        L.sah_destroy(h)
    assert n > 100


@pytest.mark.parametrize("seed", [53])
def test_no_argument_combination_crashes_the_entry(seed):
    stdout = support.run_fuzz_child("sun_shafts_fuzz_child.py", seed, 2000)
    assert not re.search(r"\bok: \d", stdout)  # (a detached context never launches)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_what_the_restatement_gives():
    fx = np.load(gen.FIXTURE)
    fx = {k: fx[k] for k in fx.files}
    fresh = gen.inputs()
    for k, v in fresh.items():
        assert fx[k].dtype == v.dtype and fx[k].tobytes() == v.tobytes(), k
    out, march = gen.outputs(fx)
    for i, (o, m) in enumerate(zip(out, march)):
        assert fx["out"][i].tobytes() == o.tobytes() and fx[f"march{i}"].tobytes() == m.tobytes(), gen.CASES[i]
        assert (o != fx["lit"]).any(-1).mean() > 0.9  # the case does something
    assert os.path.getsize(gen.FIXTURE) < (1 << 20)


# ---- properties of the restatement ------------------------------------------------------------------------------------------------------------
SW, SH = 48, 40


@pytest.fixture(scope="module")
def world():
    view = ref.scene_view(SW, SH)
    return dict(view=view.gpu_data, sun=ref.scene_sun(view), depth=ref.box_depth(SW, SH, holes=False), lit=ref.textured_lit(SW, SH, 2),
                noise=ref.noise_map(4, 64, 3, block=4))


MEDIUM = gen.MEDIUM


def test_a_a_step_transmittance_of_one_returns_lits_bits_whatever_the_map(world):
    for shadow in (world["noise"], ref.constant_map(2, 8, 0), None):
        for s in (1, 2):
            out, info = ref.sun_shafts_ex(world["view"], world["sun"], shadow, world["depth"], world["lit"], **dict(MEDIUM, step_transmittance=1.0, downscale=s, flags=ref.DITHER))
            assert out.tobytes() == world["lit"].tobytes() and (info["E"] == 0).all() and (info["T"] == 1).all()


def test_b_without_a_map_the_sums_are_the_scalar_loop(world):
    w, h = 24, 16
    view = ref.scene_view(w, h)
    sun = ref.scene_sun(view)
    settings = dict(MEDIUM, anisotropy=0.0, num_steps=16, step_length=0.75, step_transmittance=0.9)
    info = ref.march(view.gpu_data, sun, None, np.full((h, w), 0.008, f32), **settings)
    D = ref.step_table(0.9, 16)
    sl = f32(0.75)
    assert (info["ph"] == ref.INV_4PI).all()  # g = 0: q = 1 - 0 c = 1
    partial = 0
    for y in range(h):
        for x in range(w):
            n, E = info["L"][y, x] / sl, f32(0.0)
            for k in range(16):
                frac = f32(min(max(n - f32(k), f32(0.0)), f32(1.0)))
                partial += 0 < frac < 1
                E = f32(E + f32(frac * D[k]))
            assert E == info["E"][y, x] == info["V"][y, x]
            for c in range(3):
                S = f32(f32(E * f32(MEDIUM["ambient"][c])) + f32(f32(ref.INV_4PI * f32(sun.color[c])) * f32(f32(MEDIUM["albedo"][c]) * E)))
                assert S == info["S"][y, x, c]
    assert partial == w * h  # every ray ends inside a step (6.25 / 0.75 is no integer)


def test_c_transmittance_and_the_share_scattered_out_add_up_and_fall_with_depth(world):
    last = None
    for distance in (0.3, 1.0, 3.0, 9.0, 40.0):
        depth = np.full((SH, SW), f32(world["view"].z_near) / f32(distance), f32)
        info = ref.march(world["view"], world["sun"], world["noise"], depth, **MEDIUM)
        T, E = info["T"], info["E"]
        assert ((T >= 0) & (T <= 1)).all() and (np.abs((T + E) - f32(1.0)) <= f32(2.0 ** -23)).all()
        assert (E <= f32(1.0) - f32(0.98) ** 32 + f32(1e-6)).all()
        if last is not None:
            assert (T <= last).all() and (T < last).any()
        last = T
    assert (last < 0.6).all()  # 16 units of a medium that keeps 0.98 per half unit


def test_d_a_fully_occluded_map_leaves_the_ambient_term_exactly(world):
    info = ref.march(world["view"], world["sun"], ref.constant_map(4, 16, 0), world["depth"], **MEDIUM)
    dark = info["V"] == 0
    assert dark.mean() > 0.9 and (info["E"][dark] > 0).all()
    assert (info["S"][dark] == info["E"][dark, None] * np.array(MEDIUM["ambient"], f32)).all()


def test_e_rays_that_cross_a_walls_shadow_scatter_less(world):
    """a map whose first 32 rows hold the nearest depth (a wall between the sun and that half of the world) and whose other rows hold the
    farthest: a ray is either wholly lit, V == E, or loses light where it crosses the shadow, V < E; each class is at least a quarter of the
    frame (0.45 and 0.55 with this camera), so neither passes empty"""
    wall = np.ones((4, 64, 64), f32)
    wall[:, :32, :] = 0.0
    info = ref.march(world["view"], world["sun"], wall, world["depth"], **MEDIUM)
    lit, crossed = info["V"] == info["E"], info["V"] < info["E"]
    assert (lit | crossed).all() and lit.mean() >= 0.25 and crossed.mean() >= 0.25
    share = info["V"] / info["E"]
    assert share[crossed].max() < 1 and share[crossed].max() < share[lit].min()


def test_f_a_sky_pixel_and_a_surface_at_the_clip_distance_agree(world):
    d_min = f32(world["view"].z_near) / (f32(0.5) * f32(32))
    for tiny in (0.0, np.nan, -1.0, 1e-40, float(d_min)):
        a = ref.sun_shafts(world["view"], world["sun"], world["noise"], np.full((SH, SW), tiny, f32), world["lit"], **MEDIUM)
        b = ref.sun_shafts(world["view"], world["sun"], world["noise"], np.full((SH, SW), d_min, f32), world["lit"], **MEDIUM)
        assert a.tobytes() == b.tobytes() and a.tobytes() != world["lit"].tobytes()


def test_g_the_upsample_is_bilinear_on_a_plane_and_keeps_to_its_side_of_a_depth_step(world):
    """Constant depth: every depth weight is 1 / (1 + 0) = 1, the sum of the bilinear weights is exactly 1, and the result is the plain
    bilinear of the march plane.  A step of 100 : 1 in view depth: the worst pixel has odd coordinates at the inside corner of the far
    region, one tap of bilinear weight 1/4 on its own side and three on the near side, each scaled by 1 / (1 + depth_sharpness * 0.99):
    with the default 50 that is 1 / 50.5, so the pixel's own side keeps (1/4) / (1/4 + (3/4) / 50.5) = 0.944 of the weight, above the 0.9
    asked for; the bound follows from the default, not from a run."""
    z_near = f32(world["view"].z_near)
    sharp = ref.DEFAULTS["depth_sharpness"]
    assert 0.25 / (0.25 + 0.75 / (1 + sharp * 0.99)) > 0.9
    g = np.random.default_rng(3)
    march_bits = ref.to_half_bits(g.uniform(0.0, 2.0, (SH // 2, SW // 2, 4)))
    flat = np.full((SH, SW), 0.01, f32)
    term = ref.composite(march_bits, flat, None, z_near, downscale=2, flags=ref.TERM_ONLY)
    st = ref.h2f(march_bits)
    y, x = np.meshgrid(np.arange(SH), np.arange(SW), indexing="ij")
    X0, Y0 = x >> 1, y >> 1
    X1, Y1 = np.minimum(X0 + 1, SW // 2 - 1), np.minimum(Y0 + 1, SH // 2 - 1)
    fx, fy = ((x & 1) * f32(0.5))[..., None], ((y & 1) * f32(0.5))[..., None]
    plain = ((((1 - fx) * (1 - fy)) * st[Y0, X0] + (fx * (1 - fy)) * st[Y0, X1]) + ((1 - fx) * fy) * st[Y1, X0]) + (fx * fy) * st[Y1, X1]
    assert term.tobytes() == ref.to_half_bits(plain.astype(f32)).tobytes()
    even = (x % 2 == 0) & (y % 2 == 0)
    assert (term[even] == march_bits[Y0[even], X0[even]]).all()  # a pixel a texel stands for takes that texel
    stepped = np.full((SH, SW), z_near / f32(1.0), f32)
    stepped[:SH // 2, :SW // 2] = z_near / f32(100.0)  # the far region ends on odd coordinates: its corner pixel is the worst case
    d_min = f32(1e-9)
    Xs, Ys, Wt = ref.upsample_weights(stepped, z_near, d_min, sharp, SW // 2, SH // 2)
    total = sum(Wt)
    own = sum(np.where(stepped[2 * Ys[j >> 1], 2 * Xs[j & 1]] == stepped, Wt[j], 0) for j in range(4))
    assert (own / total >= 0.9).all() and (own / total < 0.95).any()


def test_h_the_dither_offset_permutes_the_sixteen_offsets():
    my, mx = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    levels = (np.arange(16, dtype=f32) + f32(0.5)) * f32(0.0625)
    seen = []
    for offset in range(16):
        o = ref.dither(mx, my, offset, ref.DITHER)
        assert sorted(o[:4, :4].ravel().tolist()) == levels.tolist() and (o[:4, :4] == o[4:, 4:]).all()
        seen.append(o)
    assert all(sorted(np.stack(seen)[:, j, i].tolist()) == levels.tolist() for j in range(4) for i in range(4))  # a texel sees all sixteen over sixteen frames
    assert (ref.dither(mx, my, 7, 0) == 0.5).all()
