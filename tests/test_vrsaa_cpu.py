"""The VRSAA passes (include/sah_vrsaa.h) without a GPU: the exports and the header, the 92-byte uniform block, every refusal the header
lists, and the restatements — a scalar one below, loop for loop like the shaders, against the vectorised one of tests/vrsaa_ref.py and
the committed fixture, plus points one can work out by hand."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from androidrenderer_amd import _abi, lib, scene
from tests import vrsaa_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_vrsaa as gen  # noqa: E402

f32 = np.float32


# ---- the scalar restatement: contrast_detection.comp:15-68 and generate_shading_rate_image.comp:19-63, one pixel at a time -------------
def _max(a, b):  # oracle/math.hpp:59
    return b if (a < b or math.isnan(a)) else a


def _min(a, b):
    return b if (b < a or math.isnan(a)) else a


def _texel(n, s):
    """NEAREST, CLAMP_TO_EDGE: texcoord = float(s) / n, index floor(texcoord * n) clamped (oracle/texture.hpp:39-43)"""
    uv = f32(s) / f32(n)
    return min(max(int(math.floor(uv * f32(n))), 0), n - 1)


def scalar_contrast(color, depth):
    h, w = depth.shape
    lut = ref.srgb_lut()
    sobel_x = ((1, 0, -1), (2, 0, -2), (1, 0, -1))  # mat3 columns
    sobel_y = ((1, 2, 1), (0, 0, 0), (-1, -2, -1))
    out = np.zeros((h, w, 2), np.float16)
    tx = [[_texel(w, px + x - 1) for x in range(3)] for px in range(w)]
    ty = [[_texel(h, py + y - 1) for y in range(3)] for py in range(h)]
    with np.errstate(all="ignore"):
        for py in range(h):
            for px in range(w):
                lg = [f32(0), f32(0)]
                for y in range(3):
                    for x in range(3):
                        c = color[ty[py][y], tx[px][x]]
                        luma = (lut[c[0]] * f32(0.2126) + lut[c[1]] * f32(0.7152)) + lut[c[2]] * f32(0.0722)
                        lg[0] = lg[0] + luma * f32(sobel_x[x][y])
                        lg[1] = lg[1] + luma * f32(sobel_y[x][y])
                dg = [f32(0), f32(0)]
                for y in range(3):
                    for x in range(3):
                        d = depth[ty[py][y], tx[px][x]]
                        dg[0] = dg[0] + d * f32(sobel_x[x][y])
                        dg[1] = dg[1] + d * f32(sobel_y[x][y])
                for k in range(2):
                    out[py, px, k] = np.float16(_max(lg[k] * f32(0.5), dg[k]))
    return out.view(np.uint16)


def scalar_shading_rate_image(contrast_bits, params):
    cw, ch = params.contrast_image_resolution
    sw, sh = params.shading_rate_image_resolution
    g = contrast_bits.view(np.float16)
    out = np.zeros((sh, sw), np.uint8)
    delta = max(1, int(np.rint(f32(cw) / f32(sw))))
    with np.errstate(all="ignore"):
        for py in range(sh):
            for px in range(sw):
                m = [f32(0), f32(0)]
                for i in range(delta):
                    for j in range(delta):
                        x, y = delta * px + i, delta * py + j
                        t = g[y, x] if (x < cw and y < ch) else (np.float16(0), np.float16(0))
                        for k in range(2):
                            v = f32(t[k])
                            m[k] = _max(m[k], abs(v * v))
                a = [_min(f32(1.25) * np.sqrt(m[k]), f32(1)) for k in range(2)]
                max_rate = f32(max(params.max_rate[0], params.max_rate[1]))
                opt = [a[k] * f32(1) + (f32(1) - a[k]) * max_rate for k in range(2)]
                index, cost = 0, f32(1) + f32(2) * max_rate * max_rate
                for i in range(params.num_shading_rates):
                    rx, ry = params.rates[i]
                    c = (f32(rx) - opt[0]) * (f32(rx) - opt[0]) + (f32(ry) - opt[1]) * (f32(ry) - opt[1])
                    if c < cost:
                        cost, index = c, i
                rx, ry = params.rates[index]
                out[py, px] = ((ry >> 1) | ((rx << 1) & 12)) & 0xff
    return out


# ---- exports, header, struct ----------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries_its_header_declares():
    L = lib.load()
    assert all(hasattr(L, s) for s in lib.VRSAA_EXPORTS)
    header = open(os.path.join(ROOT, "include", "sah_vrsaa.h")).read()
    assert sorted(re.findall(r"^int (sah_\w+)\(", header, re.M)) == sorted(lib.VRSAA_EXPORTS) == ["sah_vrsaa_measure_aliasing", "sah_vrsaa_shading_rate_image"]
    assert not set(lib.VRSAA_EXPORTS) & set(lib.EXPORTS)
    assert "vrsaa" not in open(os.path.join(ROOT, "include", "sah_hip.h")).read()  # sah_hip.h and its ABI version stay as they are
    assert "parity unpinned" in header.lower() and header.count("ABI-defined") >= 4


@pytest.mark.parametrize("language", ["c", "c++"])
def test_header_compiles_and_the_uniform_block_is_92_bytes(tmp_path, language):
    src = tmp_path / ("use.c" if language == "c" else "use.cpp")
    check = "_Static_assert" if language == "c" else "static_assert"
    src.write_text('#include "sah_vrsaa.h"\n'
                   f'{check}(sizeof(sah_shading_rate_params) == 92, "ShadingRateParams");\n'
                   f'{check}(SAH_FORMAT_R8_UINT == 13, "VK_FORMAT_R8_UINT");\n'
                   "int use(sah_ctx* c, const sah_plane* p, const sah_shading_rate_params* s) {\n"
                   "    return sah_vrsaa_measure_aliasing(c, p, p, p, 0, 0) + sah_vrsaa_shading_rate_image(c, p, p, s);\n}\n")
    clang = "/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else "cc"
    subprocess.check_call([clang, "-x", language, "-std=c11" if language == "c" else "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)], timeout=120)
    assert C.sizeof(_abi.ShadingRateParams) == 92 and _abi.FORMAT_R8_UINT == 13 and _abi.FORMAT_BPP[13] == 1


def test_shading_rate_params_fills_max_rate_and_pads_to_eight():
    p = scene.shading_rate_params((97, 61), (13, 8), ref.RATES)
    assert list(p.contrast_image_resolution) == [97, 61] and list(p.shading_rate_image_resolution) == [13, 8]
    assert list(p.max_rate) == [4, 4] and p.num_shading_rates == 7
    assert [tuple(r) for r in p.rates] == ref.RATES + [(0, 0)]
    assert list(scene.shading_rate_params((4, 4), (1, 1), [(1, 4), (2, 1)]).max_rate) == [2, 4]  # per component
    assert scene.shading_rate_image_extent((97, 61), (8, 8)) == (13, 8) and scene.shading_rate_image_extent((7680, 4320), (16, 16)) == (480, 270)
    with pytest.raises(ValueError):
        scene.shading_rate_params((4, 4), (1, 1), [(1, 1)] * 9)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
OK, INVALID, FORMAT = "well-formed", _abi.SAH_ERR_INVALID_ARGUMENT, _abi.SAH_ERR_UNSUPPORTED_FORMAT


def _plane(base, fmt, w, h, pitch=None, ptr=True, offset=0):
    return _abi.Plane((base + offset) if ptr else None, w, h, w * _abi.FORMAT_BPP.get(fmt, 4) if pitch is None else pitch, fmt)


def _measure_cases(base):
    W, H = 24, 16
    def planes(**kw):
        p = {"color": _plane(base, _abi.FORMAT_R8G8B8A8_SRGB, W, H), "depth": _plane(base + (1 << 16), _abi.FORMAT_D32_SFLOAT, W, H),
             "contrast": _plane(base + (2 << 16), _abi.FORMAT_R16G16_SFLOAT, W, H)}
        p.update(kw)
        return [p["color"], p["depth"], p["contrast"]]
    yield "whole", planes(), (0, 0), OK
    yield "band", planes(), (3, 9), OK
    yield "empty band", planes(), (5, 5), OK
    for i, name in enumerate(("color", "depth", "contrast")):
        fmt = (_abi.FORMAT_R8G8B8A8_SRGB, _abi.FORMAT_D32_SFLOAT, _abi.FORMAT_R16G16_SFLOAT)[i]
        off = base + (i << 16)
        p = planes()
        p[i] = None
        yield f"{name}: null plane", p, (0, 0), INVALID
        yield f"{name}: null pointer", planes(**{name: _plane(off, fmt, W, H, ptr=False)}), (0, 0), INVALID
        yield f"{name}: wrong format", planes(**{name: _plane(off, _abi.FORMAT_R32_SFLOAT, W, H)}), (0, 0), FORMAT
        yield f"{name}: short pitch", planes(**{name: _plane(off, fmt, W, H, pitch=W * 4 - 4)}), (0, 0), INVALID
        yield f"{name}: zero width", planes(**{name: _plane(off, fmt, 0, H)}), (0, 0), INVALID
        yield f"{name}: zero height", planes(**{name: _plane(off, fmt, W, 0)}), (0, 0), INVALID
        yield f"{name}: other width", planes(**{name: _plane(off, fmt, W - 1, H)}), (0, 0), INVALID
        yield f"{name}: other height", planes(**{name: _plane(off, fmt, W, H + 1)}), (0, 0), INVALID
        yield f"{name}: misaligned pointer", planes(**{name: _plane(off, fmt, W, H, offset=2)}), (0, 0), INVALID
        yield f"{name}: pitch not a multiple of 4", planes(**{name: _plane(off, fmt, W, H, pitch=W * 4 + 2)}), (0, 0), INVALID
    yield "contrast as UNORM colour", planes(color=_plane(base, _abi.FORMAT_R8G8B8A8_UNORM, W, H)), (0, 0), FORMAT
    yield "row_begin > row_end", planes(), (9, 3), INVALID
    yield "row_end > H", planes(), (0, H + 1), INVALID


def _rate_cases(base):
    CW, CH, SW, SH = 40, 24, 5, 3
    def call(contrast=None, sri=None, **kw):
        c = _plane(base, _abi.FORMAT_R16G16_SFLOAT, CW, CH) if contrast is None else contrast
        s = _plane(base + (1 << 16), _abi.FORMAT_R8_UINT, SW, SH) if sri is None else sri
        p = scene.shading_rate_params((CW, CH), (SW, SH), ref.RATES)
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        return [c, s, p]
    yield "plain", call(), OK
    yield "eight rates", call(num_shading_rates=8), OK
    yield "no rates", call(num_shading_rates=0), OK
    yield "padded target", call(sri=_plane(base + (1 << 16), _abi.FORMAT_R8_UINT, SW, SH, pitch=SW + 3)), OK
    yield "nine rates", call(num_shading_rates=9), INVALID
    yield "contrast resolution differs", call(contrast_image_resolution=[CW, CH + 1]), INVALID
    yield "contrast resolution differs in x", call(contrast_image_resolution=[CW - 1, CH]), INVALID
    yield "target resolution differs", call(shading_rate_image_resolution=[SW + 1, SH]), INVALID
    yield "target resolution differs in y", call(shading_rate_image_resolution=[SW, SH - 1]), INVALID
    a = call()
    yield "null contrast", [None, a[1], a[2]], INVALID
    yield "null target", [a[0], None, a[2]], INVALID
    yield "null params", [a[0], a[1], None], INVALID
    yield "contrast: null pointer", call(contrast=_plane(base, _abi.FORMAT_R16G16_SFLOAT, CW, CH, ptr=False)), INVALID
    yield "target: null pointer", call(sri=_plane(base, _abi.FORMAT_R8_UINT, SW, SH, ptr=False)), INVALID
    yield "contrast: wrong format", call(contrast=_plane(base, _abi.FORMAT_R16G16B16A16_SFLOAT, CW, CH)), FORMAT
    yield "target: R8_UNORM", call(sri=_plane(base + (1 << 16), _abi.FORMAT_R8_UNORM, SW, SH)), FORMAT
    yield "contrast: short pitch", call(contrast=_plane(base, _abi.FORMAT_R16G16_SFLOAT, CW, CH, pitch=CW * 4 - 4)), INVALID
    yield "target: short pitch", call(sri=_plane(base + (1 << 16), _abi.FORMAT_R8_UINT, SW, SH, pitch=SW - 1)), INVALID
    yield "contrast: zero extent", call(contrast=_plane(base, _abi.FORMAT_R16G16_SFLOAT, 0, CH), contrast_image_resolution=[0, CH]), INVALID
    yield "target: zero extent", call(sri=_plane(base + (1 << 16), _abi.FORMAT_R8_UINT, SW, 0), shading_rate_image_resolution=[SW, 0]), INVALID
    yield "contrast: misaligned", call(contrast=_plane(base, _abi.FORMAT_R16G16_SFLOAT, CW, CH, offset=2)), INVALID


def test_every_refusal_of_the_header_on_a_context_without_a_device():
    """A malformed call answers its status; a well-formed one gets as far as selecting the device, which a detached context does not have
    (SAH_ERR_HIP) — so nothing is launched and the made-up addresses are never used."""
    L = lib.load()
    h = lib.create_detached()
    if h is None:
        pytest.skip("a HIP device is present (made-up addresses must not reach a GPU); tests/test_vrsaa_gpu.py checks the refusals there")
    base = 0x10000000
    ref_of = lambda a: None if a is None else C.byref(a)  # noqa: E731
    n = 0
    try:
        for name, planes, rows, want in _measure_cases(base):
            got = L.sah_vrsaa_measure_aliasing(h, *[ref_of(p) for p in planes], *rows)
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"measure_aliasing, {name}: status {got}"
            n += 1
        for name, args, want in _rate_cases(base):
            got = L.sah_vrsaa_shading_rate_image(h, *[ref_of(a) for a in args])
            assert got == (_abi.SAH_ERR_HIP if want == OK else want), f"shading_rate_image, {name}: status {got}"
            n += 1
        ok = next(_measure_cases(base))[1]
        assert L.sah_vrsaa_measure_aliasing(None, *[C.byref(p) for p in ok], 0, 0) == INVALID
        ok = next(_rate_cases(base))[1]
        assert L.sah_vrsaa_shading_rate_image(None, *[C.byref(a) for a in ok]) == INVALID
    finally:
        L.sah_destroy(h)
    assert n > 50


# ---- restatements and fixture -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(gen.FIXTURE)


def test_generator_reproduces_the_committed_fixture(fixture):
    got = gen.generate(int(fixture["seed"]))
    assert sorted(got) == sorted(fixture.files)
    for k in fixture.files:
        assert np.asarray(got[k]).dtype == fixture[k].dtype and np.asarray(got[k]).tobytes() == fixture[k].tobytes(), k
    assert fixture["contrast"].shape == (61, 97, 2) and fixture["shading_rate_image"].shape == (8, 13)
    assert os.path.getsize(gen.FIXTURE) < 100 * 1024
    # what the inputs are meant to hold: the special depth values, one on a low-landing column and one on the border
    bits = fixture["depth"].view(np.uint32)
    assert {int(bits[y, x]) for x, y, _ in gen.PLANTED} == {0x7f800000, 0xff800000, 0x7fc00000, 0x80000000, 0x00000123}
    assert any(x in ref.low_landing(97) for x, _, _ in gen.PLANTED) and any(x in (0, 96) or y in (0, 60) for x, y, _ in gen.PLANTED)
    assert (fixture["contrast"] == 0x7c00).any() and not np.isnan(fixture["contrast"].view(np.float16)).any()
    assert len(np.unique(fixture["shading_rate_image"])) >= 4


def test_scalar_restatement_equals_the_vectorised_one_and_the_fixture(fixture):
    contrast = scalar_contrast(fixture["color"], fixture["depth"])
    assert contrast.tobytes() == ref.contrast(fixture["color"], fixture["depth"]).tobytes() == fixture["contrast"].tobytes()
    params = scene.shading_rate_params((97, 61), gen.SRI_EXTENT, [tuple(r) for r in fixture["rates"]])
    sri = scalar_shading_rate_image(contrast, params)
    assert sri.tobytes() == ref.shading_rate_image(fixture["contrast"], gen.SRI_EXTENT, ref.RATES).tobytes() == fixture["shading_rate_image"].tobytes()


def test_low_landing_columns_recomputed():
    """fl(fl(s / n) * n) < s, recomputed with scalar float32 arithmetic"""
    def low(n):
        return [s for s in range(n) if _texel(n, s) == s - 1]
    assert low(97) == ref.low_landing(97) and len(low(97)) == 33 and low(97)[:6] == [1, 2, 4, 7, 8, 13]
    assert low(61) == ref.low_landing(61) == [1, 2, 4, 8, 16, 32]
    assert len(ref.low_landing(3840)) == 53 and len(ref.low_landing(7680)) == 104
    assert ref.low_landing(48) == [] and ref.low_landing(119) == []
    for n in (97, 61, 3840):
        assert all(_texel(n, s) in (s, s - 1) for s in range(n)) and _texel(n, -1) == 0 and _texel(n, n) == n - 1


def test_a_vertical_step_edge_under_the_swapped_names():
    """Left half dark, right half white, no low-landing columns (width 48): sobel_x[x][y] = {1, 2, 1}[x] * {1, 0, -1}[y] differences ROWS, so
    g.x = 0 and g.y = (1 + 2 + 1) * (left - right) at the edge — the 'x' matrix does not see a vertical edge, the 'y' matrix does.  Depth
    carries the same edge with the other sign, so that max() lets both through: luma gives -4 * 0.5 (loses to depth's 0 off the edge and
    to +4 on it)."""
    W, H = 48, 8
    color = np.zeros((H, W, 4), np.uint8)
    color[:, 24:, :3] = 255
    lum = ref.gradients(ref.luma(color))
    white = ref.luma(np.full((1, 1, 4), 255, np.uint8))[0, 0]
    assert (lum[..., 0] == 0).all()
    assert (lum[:, 23:25, 1] == -(white + white + white + white)).all() and (lum[:, :23, 1] == 0).all() and (lum[:, 25:, 1] == 0).all()
    depth = np.zeros((H, W), f32)
    depth[:, :24] = 1.0  # falls to the right: +4 under {1, 0, -1}[x]
    out = ref.contrast(color, depth).view(np.float16)
    assert (out[..., 0] == 0).all() and (out[:, 23:25, 1] == 4).all() and (out[:, :23, 1] == 0).all()
    # a horizontal edge is what the 'x' matrix measures
    rows = np.zeros((8, 48), f32)
    rows[:4] = 1.0
    out = ref.contrast(np.zeros((8, 48, 4), np.uint8), rows).view(np.float16)
    assert (out[3:5, :, 0] == 4).all() and (out[..., 1] == 0).all()


def test_zero_weight_products_are_part_of_the_sum():
    depth = np.full((8, 8), 0.5, f32)  # (a power of two: no tap lands low)
    depth[3, 3] = np.inf
    out = ref.gradients(depth)
    assert np.isnan(out[3, 3]).all()  # the centre tap has weight 0 in both matrices: inf * 0
    assert np.isnan(out[3, 2, 0]) and np.isnan(out[2, 3, 1])  # and in one of them for the four edge neighbours
    assert out[3, 2, 1] == -np.inf and out[2, 3, 0] == -np.inf
    got = ref.contrast(np.zeros((8, 8, 4), np.uint8), depth).view(np.float16)
    assert (got[3, 3] == 0).all() and not np.isnan(got).any()  # maxNum: the luma term (0) where the depth gradient is NaN


def test_rate_codes_of_the_seven_rates():
    assert [ref.rate_code(x, y) for x, y in ref.RATES] == [0, 1, 4, 5, 6, 9, 10]  # VkFragmentShadingRate encoding: log2(x) << 2 | log2(y)
    assert all(ref.rate_code(x, y) == (int(math.log2(x)) << 2 | int(math.log2(y))) for x, y in ref.RATES)


def test_block_size_rounds_ties_to_even():
    assert ref.block_size(20, 8) == 2 and ref.block_size(28, 8) == 4  # 2.5 -> 2, 3.5 -> 4
    assert ref.block_size(119, 8) == 15 and ref.block_size(5, 7) == 1 and ref.block_size(1, 100) == 1 and ref.block_size(97, 13) == 7
    contrast = np.zeros((20, 20, 2), np.float16)
    contrast[2, 2] = 1.0  # texel (2, 2) belongs to shading-rate texel (1, 1) when d = 2, to (0, 0) when d = 3
    sri = ref.shading_rate_image(contrast.view(np.uint16), (8, 8), ref.RATES)
    assert sri[1, 1] == 0 and (np.delete(sri.ravel(), 9) == 10).all()


def test_search_keeps_the_first_of_equal_costs_and_rates_0_without_rates():
    flat = np.zeros((4, 4, 2), np.uint16)  # m = 0: optimal = (R, R)
    assert ref.shading_rate_image(flat, (1, 1), [(2, 4), (4, 2)])[0, 0] == ref.rate_code(2, 4)  # mirrored: equal costs, the first stays
    assert ref.shading_rate_image(flat, (1, 1), [(4, 2), (2, 4)])[0, 0] == ref.rate_code(4, 2)
    assert ref.shading_rate_image(flat, (1, 1), [(2, 2), (4, 4), (4, 4)])[0, 0] == ref.rate_code(4, 4)
    assert ref.shading_rate_image(flat, (1, 1), [(2, 1), (4, 4)], num_rates=0)[0, 0] == ref.rate_code(2, 1)
    # a rate whose cost does not beat the starting 1 + 2 R^2 is not taken, nearer than rates[0] or not: index 0 stays
    assert ref.shading_rate_image(flat, (1, 1), [(4, 4), (3, 3)], max_rate=(1, 1))[0, 0] == ref.rate_code(4, 4)
