"""The filter for the RTGI ray planes (include/sah_rtgi_denoise.h) without a GPU: the export and the header, the 52-byte parameter block
and the descriptor, every refusal the header lists on a context without a device, an argument fuzz in a child process, and the numpy
restatement (tests/rtgi_denoise_ref.py) — its committed fixture with a minimum count for every planted branch, and the properties the
pass exists for: constants as fixed points, a luminance term that luminance_sigma = 0 and a short history switch off, row bands, and the
quality orderings of the design's prototype on a synthetic static scene."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib
from tests import rt_denoise_ref as mask_ref
from tests import rtgi_denoise_ref as ref
from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_rtgi_denoise as gen  # noqa: E402

f32 = np.float32
D32, RGBA16F, RG16F, RGBA32F, RG32F = (_abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16B16A16_SFLOAT, _abi.FORMAT_R16G16_SFLOAT,
                                      _abi.FORMAT_R32G32B32A32_SFLOAT, _abi.FORMAT_R32G32_SFLOAT)
HEADER = os.path.join(ROOT, "include", "sah_rtgi_denoise.h")
FIELDS = [("max_history", 0), ("min_history", 4), ("depth_tolerance", 8), ("depth_sharpness", 12), ("normal_squarings", 16), ("passes", 20),
          ("luminance_sigma", 24), ("luminance_floor", 28), ("jitter", 32), ("previous_jitter", 40), ("flags", 48)]
FORMATS = dict(ray_buffer=RGBA16F, ray_irradiance=RGBA16F, depth=D32, normals=RGBA16F, motion_vectors=RG16F, previous_depth=D32, history=RGBA32F,
               history_moments=RG32F, accum_out=RGBA32F, moments_out=RG32F, denoised_ray_buffer=RGBA16F, denoised_irradiance=RGBA16F)
NAMES = list(FORMATS)
OUTPUTS, PREVIOUS = NAMES[8:], NAMES[5:8]
ORDER = NAMES[:8]


# ---- exports, header, structs ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.RTGI_DENOISE_EXPORTS)
    header = open(HEADER).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.RTGI_DENOISE_EXPORTS) == ["sah_rtgi_denoise"]
    assert not set(lib.RTGI_DENOISE_EXPORTS) & set(lib.EXPORTS)
    hip_h = open(os.path.join(ROOT, "include", "sah_hip.h")).read()
    assert "sah_rtgi_denoise(" not in hip_h and "R32G32" not in hip_h  # sah_hip.h's declarations and formats stay
    flat = " ".join(header.replace("\n *", " ").split())
    assert "ABI-defined" in header and "Parity unpinned" in header and "Design decision" in header
    assert "a pixel's value does not depend on the row window" in flat and "never fed the filtered value" in flat and "design choices, not measurements" in flat
    assert list(_abi.RtgiDenoiseDesc.PLANES) == re.findall(r"const sah_plane\* (\w+);", header) == NAMES


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles_and_the_ctypes_structs_have_its_sizes(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    offsets = "".join(f'{check}(offsetof(sah_rtgi_denoise_params, {n}) == {o}, "{n}");\n' for n, o in FIELDS)
    offsets += "".join(f'{check}(offsetof(sah_rtgi_denoise_desc, {n}) == {8 * i}, "{n}");\n' for i, n in enumerate(NAMES))
    src.write_text('#include <stddef.h>\n#include "sah_rtgi_denoise.h"\n'
                   f'{check}(sizeof(sah_rtgi_denoise_params) == {C.sizeof(_abi.RtgiDenoiseParams)}, "sah_rtgi_denoise_params");\n'
                   f'{check}(sizeof(sah_rtgi_denoise_desc) == {C.sizeof(_abi.RtgiDenoiseDesc)}, "sah_rtgi_denoise_desc");\n'
                   f'{check}(SAH_RTGI_DENOISE_HISTORY_INVALID == 1, "flag");\n'
                   f'{check}(SAH_FORMAT_R32G32_SFLOAT == {RG32F} && SAH_FORMAT_R32G32B32A32_SFLOAT == {RGBA32F}, "formats");\n' + offsets +
                   "int use(sah_ctx* c, const sah_view_data* v, const sah_rtgi_denoise_desc* d, const sah_rtgi_denoise_params* s) { return sah_rtgi_denoise(c, v, d, s, 0, 0); }\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert C.sizeof(_abi.RtgiDenoiseParams) == 52 and C.sizeof(_abi.RtgiDenoiseDesc) == 96 and _abi.RTGI_DENOISE_HISTORY_INVALID == ref.HISTORY_INVALID == 1
    assert [(n, getattr(_abi.RtgiDenoiseParams, n).offset) for n, _ in _abi.RtgiDenoiseParams._fields_] == FIELDS
    assert _abi.FORMAT_BPP[RGBA32F] == 16 and _abi.FORMAT_BPP[RG32F] == 8
    d = _abi.RtgiDenoiseParams.default()
    got = {n: (tuple(getattr(d, n)) if n.endswith("jitter") else getattr(d, n)) for n, _ in FIELDS}
    assert got == {k: (f32(v) if isinstance(v, float) else v) for k, v in ref.DEFAULTS.items()}
    assert (d.max_history, d.min_history, d.normal_squarings, d.passes, d.luminance_sigma, d.depth_sharpness) == (32.0, 4.0, 5, 3, 4.0, 50.0)  # the issue's table
    assert abs(d.depth_tolerance - 0.1) < 1e-8 and abs(d.luminance_floor - 1e-6) < 1e-12
    assert _abi.RtgiDenoiseParams.default(passes=1, jitter=(0.5, -0.25)).jitter[1] == -0.25


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
OK, INVALID, FORMAT = "well-formed", _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT


def _plane(base, fmt, w, h, pitch=None, ptr=True, offset=0, bpp=None):
    bpp = _abi.FORMAT_BPP[fmt] if bpp is None else bpp
    return _abi.Plane((base + offset) if ptr else None, w, h, w * bpp if pitch is None else pitch, fmt)


def _view(changes=()):
    v = _abi.ViewData()
    for i in (0, 5, 10, 15):
        v.view[i] = v.inverse_view[i] = v.last_frame_view[i] = 1.0
    v.projection[0], v.projection[5], v.projection[8], v.projection[9], v.z_near = 1.2, -2.0, 0.01, -0.02, 0.05
    for k, val in dict(changes).items():
        if k == "z_near":
            v.z_near = val
        else:
            getattr(v, k[0])[k[1]] = val
    return v


def _cases(base):
    """(name, [view, desc, params], rows, expected)"""
    W, H = 24, 16
    where = {n: base + (i << 16) for i, n in enumerate(NAMES)}
    P = _abi.RtgiDenoiseParams.default
    cut = P(flags=1)

    def call(params=None, view=None, **kw):
        p = {n: _plane(where[n], FORMATS[n], W, H) for n in NAMES}
        p.update(kw)
        return [_view() if view is None else view, _abi.RtgiDenoiseDesc.of(**p), P() if params is None else params]
    yield "whole", call(), (0, 0), OK
    yield "band", call(), (3, 9), OK
    yield "empty band", call(), (5, 5), OK
    for passes in (0, 1, 2):
        yield f"passes {passes}", call(P(passes=passes)), (0, 0), OK
    yield "limits of the ranges", call(P(max_history=1.0, min_history=1.0, depth_sharpness=0.0, normal_squarings=0, luminance_sigma=0.0, luminance_floor=1e-30)), (0, 0), OK
    yield "limits of the ranges, other end", call(P(max_history=256.0, min_history=256.0, normal_squarings=7, depth_tolerance=1e30, luminance_sigma=1e30)), (0, 0), OK
    yield "padded pitches", call(depth=_plane(where["depth"], D32, W, H, pitch=W * 4 + 12), moments_out=_plane(where["moments_out"], RG32F, W, H, pitch=W * 8 + 4)), (0, 0), OK
    yield "a cut, no previous planes", call(cut, previous_depth=None, history=None, history_moments=None), (0, 0), OK
    bogus = _plane(where["history"], D32, 3, 0, ptr=False)
    yield "a cut, previous planes that are not looked at", call(cut, previous_depth=bogus, history=bogus, history_moments=bogus), (0, 0), OK
    yield "a cut, the history is accum_out's memory", call(cut, history=_plane(where["accum_out"], RGBA32F, W, H)), (0, 0), OK
    yield "params NULL", call()[:2] + [None], (0, 0), INVALID
    yield "desc NULL", [_view(), None, P()], (0, 0), INVALID
    yield "view NULL", [None] + call()[1:], (0, 0), INVALID
    for n in NAMES:
        fmt, bpp = FORMATS[n], _abi.FORMAT_BPP[FORMATS[n]]
        yield f"{n}: null plane", call(**{n: None}), (0, 0), INVALID
        yield f"{n}: null pointer", call(**{n: _plane(where[n], fmt, W, H, ptr=False)}), (0, 0), INVALID
        other = D32 if fmt != D32 else _abi.FORMAT_R32_SFLOAT
        yield f"{n}: wrong format", call(**{n: _plane(where[n], other, W, H, bpp=bpp)}), (0, 0), FORMAT
        yield f"{n}: short pitch", call(**{n: _plane(where[n], fmt, W, H, pitch=W * bpp - 4)}), (0, 0), INVALID
        yield f"{n}: zero width", call(**{n: _plane(where[n], fmt, 0, H)}), (0, 0), INVALID
        yield f"{n}: zero height", call(**{n: _plane(where[n], fmt, W, 0)}), (0, 0), INVALID
        yield f"{n}: other width", call(**{n: _plane(where[n], fmt, W - 2, H)}), (0, 0), INVALID
        yield f"{n}: other height", call(**{n: _plane(where[n], fmt, W, H + 1, pitch=W * bpp)}), (0, 0), INVALID
        yield f"{n}: misaligned pointer", call(**{n: _plane(where[n], fmt, W, H, offset=2)}), (0, 0), INVALID
        yield f"{n}: pitch not a multiple of 4", call(**{n: _plane(where[n], fmt, W, H, pitch=W * bpp + 2)}), (0, 0), INVALID
    yield "row_begin > row_end", call(), (9, 3), INVALID
    yield "row_end > H", call(), (0, H + 1), INVALID
    nan, inf = float("nan"), float("inf")
    for field in ("max_history", "min_history"):
        for v in (0.999, 0.0, -1.0, 256.5, inf, nan):
            yield f"{field} {v}", call(P(**{field: v})), (0, 0), INVALID
    for field in ("depth_tolerance", "luminance_floor"):
        for v in (0.0, -0.1, inf, nan):
            yield f"{field} {v}", call(P(**{field: v})), (0, 0), INVALID
    for field in ("depth_sharpness", "luminance_sigma"):
        for v in (-0.001, inf, -inf, nan):
            yield f"{field} {v}", call(P(**{field: v})), (0, 0), INVALID
    for v in (8, 0xffffffff):
        yield f"normal_squarings {v}", call(P(normal_squarings=v)), (0, 0), INVALID
    for v in (4, 0xffffffff):
        yield f"passes {v}", call(P(passes=v)), (0, 0), INVALID
    for flags in (2, 3, 0x80000000):
        yield f"flags {flags:#x}", call(P(flags=flags)), (0, 0), INVALID
    for field in ("jitter", "previous_jitter"):
        for v in ((nan, 0.0), (0.0, inf), (-inf, 0.0)):
            yield f"{field} {v}", call(P(**{field: v})), (0, 0), INVALID
    read = [("projection", i) for i in (0, 5, 8, 9)] + [("inverse_view", i) for i in (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14)] + \
           [("last_frame_view", i) for i in (2, 6, 10, 14)] + ["z_near"]
    for key in read:
        yield f"NaN in {key}", call(view=_view({key: nan})), (0, 0), INVALID
    for key in [("projection", i) for i in (1, 2, 3, 4, 10, 14)] + [("view", i) for i in range(16)] + [("inverse_view", i) for i in (3, 7, 11, 15)] + \
               [("last_frame_view", i) for i in (0, 1, 3, 4, 5, 12, 13, 15)]:
        yield f"NaN in {key}, which is not read", call(view=_view({key: nan})), (0, 0), OK
    for z_near in (0.0, -0.05, inf):
        yield f"z_near {z_near}", call(view=_view({"z_near": z_near})), (0, 0), INVALID
    # the byte ranges of the four targets against the inputs' and each other's
    size = {n: H * W * _abi.FORMAT_BPP[FORMATS[n]] for n in NAMES}
    for target in OUTPUTS:
        fmt = FORMATS[target]
        for n in [m for m in NAMES if m != target]:
            yield f"{target} is {n}'s memory", call(**{target: _plane(where[n], fmt, W, H)}), (0, 0), INVALID
            yield f"{target} ends inside {n}", call(**{target: _plane(where[n] - size[target] + 4, fmt, W, H)}), (0, 0), INVALID
            yield f"{target} begins inside {n}", call(**{target: _plane(where[n] + size[n] - 4, fmt, W, H)}), (0, 0), INVALID
            yield f"{target} ends where {n} begins", call(**{target: _plane(where[n] - size[target], fmt, W, H)}), (0, 0), OK


def test_every_refusal_of_the_header_on_a_context_without_a_device():
    """A malformed call answers its status; a well-formed one gets as far as selecting the device, which a detached context does not have
    (SAH_ERR_HIP) — so nothing is launched and the made-up addresses are never used."""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present (made-up addresses must not reach a GPU); tests/test_rtgi_denoise_gpu.py checks the refusals there")
    ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
    n = 0
    try:
        for name, args, rows, want in _cases(0x10000000):
            got = L.sah_rtgi_denoise(h, *[ref_of(a) for a in args], *rows)
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"{name}: status {got}"
            n += 1
        ok = next(_cases(0x10000000))[1]
        assert L.sah_rtgi_denoise(None, *[C.byref(a) for a in ok], 0, 0) == INVALID
    finally:
        L.sah_destroy(h)
    assert n > 350


@pytest.mark.parametrize("seed", [11, 12])
def test_argument_fuzz_in_a_child_process(seed):
    """random bits in every argument (tests/rtgi_denoise_fuzz_child.py): every call comes back with a sah_status and the process survives"""
    stdout = support.run_fuzz_child("rtgi_denoise_fuzz_child.py", seed, 2000)
    assert " ok:" not in stdout and "invalid_argument:" in stdout and "hip:" in stdout  # (a detached context never launches; well-formed calls get as far as the device)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(gen.FIXTURE))


def _run(inputs, view, settings):
    return ref.denoise_ex(*[inputs.get(k) for k in ORDER], view, settings)


def test_fixture_reproduces_and_is_small(fixture):
    again = gen.generate(int(fixture["seed"]))
    assert set(again) == set(fixture)
    for k in again:
        assert np.asarray(again[k]).tobytes() == fixture[k].tobytes() and np.asarray(again[k]).dtype == fixture[k].dtype, k
    assert os.path.getsize(gen.FIXTURE) < 200 * 1024 and (gen.WIDTH, gen.HEIGHT, gen.FRAMES) == (69, 21, 3)
    assert not [k for k in fixture if k.startswith(("accum", "moments")) and "passes" in k]  # the accumulation planes once per frame


def test_fixture_takes_every_planted_branch(fixture):
    count = lambda m: int(np.sum(m))  # noqa: E731
    runs = [_run(gen.frame_of(fixture, i), gen.view(i), gen.params(i, 3)) for i in range(3)]
    depth = fixture["depth"]
    sky = ~runs[0][4]["ok"]
    assert count(depth == 0) >= 290 and count(np.isnan(depth)) == 3 and count(depth < 0) == 3 and count(sky) == count(~(depth > 0)) + 5  # (one of the planted normals lies in the sky)
    for i, (accum, moments, drb, dirr, info) in enumerate(runs):
        # a pixel without a surface copies both inputs and stores zeros
        assert drb[sky].tobytes() == fixture[f"ray_buffer{i}"][sky].tobytes() and dirr[sky].tobytes() == fixture[f"ray_irradiance{i}"][sky].tobytes()
        assert not accum[sky].any() and not moments[sky].any() and (accum[~sky][:, 3] >= 1).all()
        assert count(info["nonfinite_sample"]) >= 3 and np.isfinite(accum[~sky]).all() and np.isfinite(info["value"][~sky]).all()
        assert (dirr[~sky][:, 3] == 0).all() and drb[~sky][:, 3].tobytes() == fixture[f"ray_buffer{i}"][~sky][:, 3].tobytes()
        assert count(info["sample"].any(-1)) >= 150  # a third of the rays carry light, and most of those leave the surface's side
        assert fixture[f"accum{i}"].tobytes() == accum.tobytes() and fixture[f"moments{i}"].tobytes() == moments.tobytes()
        assert fixture[f"denoised_irradiance{i}_passes3"].tobytes() == dirr.tobytes()
    i0, i1, i2 = (r[4] for r in runs)
    assert fixture["denoised_ray_buffer0"].tobytes() == runs[0][2].tobytes()
    # frame 0: no history anywhere, so every pixel is short and the luminance term is off
    assert count(i0["history"]) == 0 and set(np.unique(runs[0][0][..., 3]).tolist()) == {0.0, 1.0}
    assert not any(fi["luminance_active"].any() for fi in i0["filter"])
    # frame 1
    assert count(i1["history"] & (i1["taps_valid"] == 1)) >= 700        # a static camera: its own texel
    assert count(i1["taps_valid"] == 4) >= 30                           # sub-pixel motion: four taps
    assert count(i1["q_outside"]) >= 100 and count(i1["tap_outside"]) >= 8
    assert count(i1["bad_history_texel"]) >= 9                          # the NaN colours, the zero counts and the inf moments
    assert count(i1["depth_rejected"]) >= 50 and count(i1["depth_rejected"] & (i1["taps_valid"] > 0)) >= 10
    assert count(i1["no_tap"]) >= 40
    n1 = runs[1][0][..., 3]
    assert (n1[i1["history"]] == 2).all() and (n1[i1["ok"] & ~i1["history"]] == 1).all()
    # min_history = 2: the term is active exactly where there is a history, and it changes the result
    for fi in i1["filter"]:
        assert (fi["luminance_active"] == i1["history"]).all() and count(fi["luminance_active"]) >= 700 and count(i1["ok"] & ~fi["luminance_active"]) >= 100
    geometry_only = _run(gen.frame_of(fixture, 1), gen.view(1), dict(gen.params(1, 3), luminance_sigma=0.0))[3]
    assert count((geometry_only != runs[1][3]).any(-1)) >= 500
    # frame 2: the dolly — the near band's history fails the depth test, the others keep theirs
    xx = np.mgrid[0:gen.HEIGHT, 0:gen.WIDTH][1]
    ok = i2["ok"]
    assert i2["history"][ok & (xx >= 24)].all() and not i2["history"][ok & (xx < 24)].any() and count(ok & (xx < 24)) >= 400
    assert set(np.unique(runs[2][0][..., 3][ok & (xx >= 24)]).tolist()) == {2.0, 3.0}
    # the irradiance edge is on a flat surface: neither depth nor normals see it
    z = i2["z"]
    edge = ok[:, gen.EDGE - 1] & ok[:, gen.EDGE]
    assert count(edge) >= 15 and (np.abs(z[:, gen.EDGE] - z[:, gen.EDGE - 1])[edge] * (f32(50) / z[:, gen.EDGE][edge]) < 0.5).all()
    # and the passes do something everywhere
    for i in range(3):
        for p in range(3):
            assert count((fixture[f"denoised_irradiance{i}_passes{p}"] != fixture[f"denoised_irradiance{i}_passes{p + 1}"]).any(-1)) >= 700


# ---- scenes for the properties ------------------------------------------------------------------------------------------------------------------
Z_NEAR = 0.05


def flat_view():
    """camera at the origin looking down -z, no jitter in the projection, a static camera"""
    return ref.View.of(1.0, 2.0, 0.0, 0.0, Z_NEAR)


def wall(w, h, z=4.0):
    """depth and normals (uint16 bits) of a fronto-parallel wall at distance z (a scalar or an (h, w) array)"""
    depth = (Z_NEAR / np.broadcast_to(np.asarray(z, np.float64), (h, w))).astype(f32)
    n = np.zeros((h, w, 4), np.float16)
    n[..., 2] = 1.0
    return depth, n.view(np.uint16)


def zeros_mv(w, h, mv=(0.0, 0.0)):
    m = np.zeros((h, w, 2), np.float16)
    m[...] = mv
    return m


def along_the_normal(irradiance):
    """rays along (0, 0, 1) — the wall's normal, so E = irr exactly — with `irradiance` (H, W, 3)"""
    h, w = irradiance.shape[:2]
    rays = np.zeros((h, w, 4), np.float16)
    rays[..., 2], rays[..., 3] = 1.0, 3.0
    irr = np.zeros((h, w, 4), np.float16)
    irr[..., :3] = irradiance
    return rays.view(np.uint16), irr.view(np.uint16)


@pytest.mark.parametrize("value", [(0.7, 0.5, 0.25), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1.0e-3, 3.0e-3, 0.0)])
def test_a_constant_field_is_a_fixed_point_bit_for_bit(value):
    """through the accumulation (a static camera and a whole-pixel pan: one tap of weight 1) and all three iterations, whatever the
    surfaces are, with the luminance term on (every history count is above min_history)"""
    W, H = 40, 24
    inputs = ref.random_inputs(W, H, 5)
    value = np.array(value, np.float16).astype(f32)
    N = ref.surfaces(inputs["depth"], inputs["normals"], flat_view())[3]
    rays = np.zeros((H, W, 4), np.float16)
    rays[..., :3] = N * 4  # dir . N >= 1 wherever there is a surface: clamp01 gives exactly 1
    irr = np.zeros((H, W, 4), np.float16)
    irr[..., :3] = value
    inputs["ray_buffer"], inputs["ray_irradiance"] = rays.view(np.uint16), irr.view(np.uint16)
    l = ref.lum(value)
    inputs["history"] = np.broadcast_to(np.concatenate([value, [f32(7)]]).astype(f32), (H, W, 4)).copy()
    inputs["history_moments"] = np.broadcast_to(np.array([l, l * l], f32), (H, W, 2)).copy()
    view = flat_view()
    for mv in ((0.0, 0.0), (2.0, -1.0)):
        inputs["motion_vectors"] = zeros_mv(W, H, mv)
        accum, moments, drb, dirr, info = _run(inputs, view, dict(passes=3))
        ok = info["ok"]
        assert info["history"].sum() > W * H // 8 and (~info["history"] & ok).any()
        assert (accum[ok][:, :3].view(np.uint32) == value.view(np.uint32)).all() and (accum[info["history"]][:, 3] == 8).all()
        assert info["filter"][0]["luminance_active"].sum() > W * H // 8
        for plane in info["planes"]:
            assert (plane[ok].view(np.uint32) == value.view(np.uint32)).all()
        assert (dirr[ok][:, :3] == value.astype(np.float16).view(np.uint16)).all()


def test_luminance_sigma_zero_removes_the_term():
    """with luminance_sigma = 0 every channel is filtered exactly as sah_rt_denoise filters its one plane: the same weights (k, dw, e), the
    same sums — bit for bit against that restatement, channel by channel, through all three iterations"""
    W, H = 61, 33
    inputs = ref.random_inputs(W, H, 3)
    view = flat_view()
    accum, moments, _, dirr, info = _run(inputs, view, dict(passes=3, luminance_sigma=0.0))
    assert not any(fi["luminance_active"].any() for fi in info["filter"])
    ok, z, _, _, M = ref.surfaces(inputs["depth"], inputs["normals"], view)
    for ch in range(3):
        v = np.ascontiguousarray(accum[..., ch])
        for i in range(3):
            v, _ = mask_ref.filter_pass_ex(v, ok, z, M, 1 << i, 50.0, 5)
        assert v[ok].tobytes() == np.ascontiguousarray(info["value"][..., ch])[ok].tobytes(), f"channel {ch}"
    with_term = _run(inputs, view, dict(passes=3))
    assert (with_term[3] != dirr).any(-1).sum() > W * H // 4 and with_term[0].tobytes() == accum.tobytes()  # the term matters, and only to the filter


def test_a_pixel_with_a_short_history_ignores_the_term():
    """one iteration: a centre pixel with n < min_history gets what luminance_sigma = 0 gives it, whatever its neighbours' counts are; with
    min_history above every count the whole result is the geometry-only one, through all three iterations"""
    W, H = 61, 33
    inputs = ref.random_inputs(W, H, 4)
    view = flat_view()
    on, off = _run(inputs, view, dict(passes=1)), _run(inputs, view, dict(passes=1, luminance_sigma=0.0))
    info = on[4]
    short, ok = info["short"], info["ok"]
    n = on[0][..., 3]
    assert (short == (ok & (n < 4))).all() and short.sum() > W * H // 8 and (ok & ~short).sum() > W * H // 8  # counts on both sides of min_history
    assert (info["filter"][0]["luminance_active"] == (ok & ~short)).all()
    assert on[3][short].tobytes() == off[3][short].tobytes()
    assert (on[3] != off[3]).any(-1)[ok & ~short].mean() > 0.5
    all_short = _run(inputs, view, dict(passes=3, min_history=256.0))
    assert all_short[3].tobytes() == _run(inputs, view, dict(passes=3, luminance_sigma=0.0))[3].tobytes()


# ---- bands ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 1, 2, 3])
def test_three_bands_reassemble_the_frame(fixture, passes):
    """a band computes accum_out and moments_out over its rows widened by 2^passes - 1 and nothing else: every row beyond is poisoned (no
    surface, NaN values) before the filter runs, and the band's rows of the denoised irradiance still equal the whole frame's"""
    inputs, view, settings = gen.frame_of(fixture, 1), gen.view(1), dict(ref.DEFAULTS, **gen.params(1, passes))
    H, W = gen.HEIGHT, gen.WIDTH
    accum, moments, drb, dirr, info = _run(inputs, view, settings)
    ok, z, _, N, M = ref.surfaces(inputs["depth"], inputs["normals"], view)
    short = accum[..., 3] < f32(settings["min_history"])
    out = np.zeros((H, W, 4), np.uint16)
    for rows in ((0, 6), (6, 7), (7, H)):
        a0, a1 = ref.band_rows(rows, H, passes)
        assert (a0, a1) == (max(rows[0] - (2 ** passes - 1), 0), min(rows[1] + (2 ** passes - 1), H))
        inside = np.zeros((H, W), bool)
        inside[a0:a1] = True
        v = np.where(inside[..., None], accum[..., :3], f32(np.nan)).astype(f32)
        var = np.where(inside, ref.variance_of(moments), f32(np.nan)).astype(f32)
        for i in range(passes):
            v, var, _ = ref.filter_pass_ex(v, var, ok & inside, z, M, short, 1 << i, settings)
        out[rows[0]:rows[1]] = ref.pack(inputs["ray_buffer"], inputs["ray_irradiance"], ok, N, v)[1][rows[0]:rows[1]]
    assert out.tobytes() == dirr.tobytes()
    assert ref.band_rows((5, 5), H, passes) == (5, 5) and ref.band_rows((0, H), H, passes) == (0, H)


# ---- what the pass is for ---------------------------------------------------------------------------------------------------------------------
def test_quality_orderings_on_a_static_scene_over_sixteen_frames():
    """96 x 48, a static camera; a wall at z = 4 with an irradiance edge at a third of the width (1.0 against 0.35, tinted), and a depth step
    to z = 6 at two thirds.  Rays along the normal carry the truth times a gamma(2) variate of mean 1: a one-ray estimator whose mean is the
    truth.  After 16 frames, RMS error against the truth over the whole image: raw > accumulated > denoised; over the strip of eight columns
    around the irradiance edge: luminance_sigma = 4 below luminance_sigma = 0 (the geometry-only filter, which blurs the edge for ever).
    Orderings only; the figures are printed.  At the time of writing: raw 0.3777, accumulated 0.0925, denoised 0.0163; strip: sigma 4
    0.0474, sigma 0 0.1634."""
    W, H = 96, 48
    xx = np.mgrid[0:H, 0:W][1]
    depth, normals = wall(W, H, np.where(xx >= 64, 6.0, 4.0))
    truth = np.where(xx < 32, 1.0, 0.35)[..., None] * np.array([1.0, 0.8, 0.6])
    g = np.random.default_rng(2026)
    view, mv = flat_view(), zeros_mv(W, H)
    accum = moments = None
    for i in range(16):
        rays, irr = along_the_normal(truth * g.gamma(2.0, 0.5, (H, W, 1)))
        last = i == 15
        accum, moments, _, dirr, info = ref.denoise_ex(rays, irr, depth, normals, mv, depth, accum, moments, view,
                                                       dict(passes=3 if last else 0, flags=0 if i else ref.HISTORY_INVALID))
    assert (accum[..., 3] == 16).all() and info["filter"][0]["luminance_active"].all()
    rms = lambda a, m=np.ones((H, W), bool): float(np.sqrt(np.mean((a.astype(np.float64) - truth)[m] ** 2)))  # noqa: E731
    value = lambda bits: bits.view(np.float16)[..., :3].astype(f32)  # noqa: E731
    raw = value(irr)
    # the geometry-only filter of the same accumulated planes (the history is never fed the filtered value: the accumulation is the same)
    ok, z, _, N, M = ref.surfaces(depth, normals, view)
    v, var = accum[..., :3].copy(), ref.variance_of(moments)
    for k in range(3):
        v, var, _ = ref.filter_pass_ex(v, var, ok, z, M, np.zeros((H, W), bool), 1 << k, dict(ref.DEFAULTS, luminance_sigma=0.0))
    geometry_only = v.astype(np.float16).astype(f32)
    strip = (xx >= 28) & (xx < 36)
    figures = dict(raw=rms(raw), accumulated=rms(accum[..., :3]), denoised=rms(value(dirr)), strip_sigma4=rms(value(dirr), strip), strip_sigma0=rms(geometry_only, strip))
    print("frame 16, RMS against the truth: " + ", ".join(f"{k} {v:.4f}" for k, v in figures.items()))
    assert figures["raw"] > figures["accumulated"] > figures["denoised"]
    assert figures["strip_sigma4"] < figures["strip_sigma0"]
